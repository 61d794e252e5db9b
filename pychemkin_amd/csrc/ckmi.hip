// ckmi.hip -- gfx950 kernels and the C ABI of libckmi.so (see include/ckmi.h).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "../../include/ckmi.h"
#include "ckmi_reactor.hpp"
#include "ckmi_run.hpp"
#include "ckmi_internal.hpp"

using namespace ckmi;

namespace {

thread_local std::string g_err;
// Kernel-path overrides (ckmi_set_reactor_path / ckmi_set_rop_path): process-wide test and A/B
// knobs, not per thread or per stream; each launch reads its selector once.
std::atomic<int> g_reactor_path{0};
std::atomic<int> g_rop_path{0};
constexpr int JIT_MIN_STATES = 16384;  // automatic choice: the specialised kernel from this batch size up

}  // namespace

// the wave-per-reactor integrator kernel and its launcher (shared with ckmi_psr.hip)
#include "ckmi_reactor_kernel.hpp"

namespace {

// ---------------------------------------------------------------- engine heat release
// Heat rates of an engine run on its saved states (KINAll0D_GetEngineHeatRelease, engine.py:953-988):
// one wave per state evaluates the integrator's own right-hand side (reactor_rhs, problem 4) there,
// so the rates are the ones the solution was integrated with, not finite differences of it:
//   ahrr  = m c_v dT/dt + P dV/dt   [erg/s]  apparent heat release (chemical heat release net of the
//                                           wall loss: the first law of the closed cylinder)
//   qloss = hA (T - T_wall)          [erg/s]  wall heat loss (ICHX / Woschni, engine_hA; 0 adiabatic)
// The per-reactor context is built from the cylinder's initial state as the reactor kernel does.
template <bool PL>
__global__ __launch_bounds__(WAVE) void engine_heat_kernel(MechImage img, const DevCfg* __restrict__ dcfg, double T0,
                                                           double P0, const double* __restrict__ Y0, int n,
                                                           const double* __restrict__ ts, const double* __restrict__ ys,
                                                           double* __restrict__ ahrr, double* __restrict__ qloss) {
  const ckmi_reactor_cfg* __restrict__ cfg = &dcfg->c;
  stage_image(0, img);
  const MechView V = make_view(0, img);
  const int lane = threadIdx.x;
  WaveLds L;
  L.base = align16(img.bytes);
  RunCtx& R = *lds_at<RunCtx>(L.base + slice_vec_bytes(img.G));
  const int KK = V.KK;
  const bool isp = lane >= 1 && lane <= KK;
  const int s = isp ? lane - 1 : 0;
  const double rw = isp ? V.rwt()[s] : 0.0;
  const double y0 = lane == 0 ? T0 : (isp ? Y0[s] : 0.0);
  const double Wbar0 = 1.0 / wave_sum(isp ? y0 * rw : 0.0);
  if (lane == 0) {
    R.cfg = cfg;
    R.pfr = 2;
    R.conp = 0;
    R.energy = cfg->energy;
    R.npv = 0;
    R.ntp = 0;
    R.rho0 = P0 * Wbar0 / (RU * T0);
    double dv;
    engine_volume(cfg->eng, 0.0, R.V0, dv);
    R.P0 = P0;
    R.mass = R.rho0 * R.V0;
    R.gfac = cfg->gfac;
    R.qloss = R.htc = R.areaq = 0.0;
    R.tamb = 300.0;
    R.nq = R.na = 0;
    R.a_t = R.a_v = nullptr;
    R.pslot = -1;
    R.plnf = 0.0;
  }
  {  // gamma of the charge (Woschni's motored pressure) and its temperature, as the reactor kernel
    const double cpR = isp ? nasa7_img(V, s, T0, log(T0), 1.0 / T0).cpR : 0.0;
    const double cpm = wave_sum(isp ? y0 * cpR * rw : 0.0);
    if (lane == 0) {
      R.G = cpm / (cpm - 1.0 / Wbar0);
      R.Pm = T0;
    }
  }
  wave_lds_sync();
  for (int i = blockIdx.x; i < n; i += gridDim.x) {
    const double t = ts[i];
    const double yl = lane <= KK ? ys[(size_t)i * (KK + 1) + lane] : 0.0;
    if (lane == 0) R.tsel = t;
    wave_lds_sync();
#ifdef CKMI_PHASE_TIMERS
    unsigned long long sub[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    const double fl = reactor_rhs<PL, true>(V, R, t, yl, L, 0, WAVE, false, nullptr, sub);
#else
    const double fl = reactor_rhs<PL, true>(V, R, t, yl, L, 0, WAVE, false, nullptr);
#endif
    const double T = bcast(yl, 0), dTdt = bcast(fl, 0);
    const double Yk = isp ? yl : 0.0;
    const double lnT = log(T);
    const Thermo7 th = isp ? nasa7_img(V, s, T, lnT, 1.0 / T) : Thermo7{0.0, 0.0, 0.0};
    const double cpk = th.cpR * RU * rw;
    const double cvm = wave_sum(Yk * (cpk - RU * rw));
    const double Wbar = 1.0 / wave_sum(Yk * rw);
    double Vc, dVdt;
    engine_volume(cfg->eng, t, Vc, dVdt);
    const double rho = R.mass / Vc;
    const double P = rho * RU * T / Wbar;
    double q = 0.0;
    if (cfg->eng[CKMI_ENG_HTMODEL] == 1.0) {  // the RHS's wall term (reactor_rhs, engine branch)
      const double cpmass = wave_sum(Yk * cpk);
      const double xp = fmax(Yk, 0.0) * rw;
      const double Tw = cfg->eng[CKMI_ENG_TWALL];
      q = engine_hA(V, R, T, log(0.5 * (T + Tw)), P, rho, Vc, xp / wave_sum(xp), cpmass, isp, s) * (T - Tw);
    }
    if (lane == 0) {
      ahrr[i] = R.mass * cvm * dTdt + P * dVdt;
      qloss[i] = q;
    }
    wave_lds_sync();  // R.tsel and the slice are rewritten for the next state
  }
}

// ---------------------------------------------------------------- ROP kernels
// Persistent grid of ROP_WAVES-wave workgroups; the workgroup stages the mechanism image in LDS
// once, each wave then takes tasks of ROP_CHUNK consecutive states and evaluates them one at a
// time (lanes over species for thermo, over reactions for the rates).  Consecutive states of one
// wave touch the same cache lines of the species-major inputs / outputs ([KK][n]), so each line
// is fetched once by one XCD and partial-line writes merge in its L2 (one state per workgroup
// spread consecutive states over all 8 XCDs: 4-8x HBM traffic, measured).
//
// Inputs and outputs of a chunk move through LDS in half-chunks of ROP_SUB states: rows T, P,
// Y_1..Y_KK of ROP_SUB consecutive states are loaded with one 64-B request per row, and the
// half-chunk's wdot_1..wdot_KK, cp, h go back the same way, so every HBM request covers whole
// 64-B halves of 128-B lines (one state at a time, lane = species, touched 53 lines with 8 B
// each: 8.8x the algorithmic traffic, measured).
//
// Mechanisms with more than 63 species (up to 255) run the same kernel with NCH = KKp / 64
// species per lane (lane + 64 j) and half as many waves per workgroup (the image, the species
// arrays and the staging rows grow with KK).
constexpr int ROP_WAVES = 8;
constexpr int ROP_CHUNK = 16;
constexpr int ROP_SUB = 8;
constexpr int ROP_LD = ROP_SUB + 1;  // odd row stride: lane = species reads of one state spread over the banks
__host__ __device__ constexpr int rop_waves(int nch) { return nch == 1 ? ROP_WAVES : 4; }
__host__ __device__ constexpr int rop_io_bytes(int KK) { return align16(8 * ROP_LD * (KK + 2)); }
__host__ __device__ constexpr int rop_slice_bytes(int G, int KK, int KKp) {
  return align16(8 * (3 * KKp + (G > 0 ? G : 1))) + rop_io_bytes(KK);
}

template <int MODE, int NCH, bool PL = false>  // MODE 0: wdot + cp + h, 1: qf / qr; NCH species per lane; PL: PLOG
__global__ __launch_bounds__(rop_waves(NCH)* WAVE) void rop_kernel(MechImage img, const int* __restrict__ orig,
                                                                  int nstate, const double* __restrict__ Tv,
                                                                  const double* __restrict__ Pv,
                                                                  const double* __restrict__ Yv,
                                                                  double* __restrict__ o0, double* __restrict__ o1,
                                                                  double* __restrict__ o2) {
  constexpr int NW = rop_waves(NCH);
  stage_image(0, img);
  const MechView V = make_view(0, img);
  const int wid = threadIdx.x / WAVE;
  const int lane = threadIdx.x % WAVE;
  const int KKp = img.KKp;
  const int slice = rop_slice_bytes(img.G, img.KK, KKp);
  const int oC = img.bytes + wid * slice;
  double* C = lds_at<double>(oC);
  double* gRT = C + KKp;
  double* wdot = gRT + KKp;
  double* Mg = wdot + KKp;
  const int KK = V.KK;
  const int sp_one = img.sp_one;
  // half-chunk staging rows [KK + 2][ROP_SUB]: T, P, Y_k in; cp, h, wdot_k out (same slots)
  double* io = lds_at<double>(oC + slice - rop_io_bytes(img.KK));
  const int nrow = KK + 2;
  const int io_c = lane & (ROP_SUB - 1), io_r = lane / ROP_SUB;
  double rw[NCH];
#pragma unroll
  for (int j = 0; j < NCH; ++j) rw[j] = lane + WAVE * j < KK ? V.rwt()[lane + WAVE * j] : 0.0;
  const int ntask = (nstate + ROP_CHUNK - 1) / ROP_CHUNK;
  for (int task = blockIdx.x * NW + wid; task < ntask; task += gridDim.x * NW) {
    const int s1 = min(nstate, (task + 1) * ROP_CHUNK);
    for (int st = task * ROP_CHUNK; st < s1; ++st) {
      const int c = st & (ROP_SUB - 1);
      const int sb = st - c;                      // first state of this half-chunk
      const int cnt = min(ROP_SUB, s1 - sb);      // states in it
      if (c == 0) {
        for (int r = io_r; r < nrow; r += WAVE / ROP_SUB) {
          double v = 0.0;
          if (io_c < cnt) v = r == 0 ? Tv[sb + io_c] : (r == 1 ? Pv[sb + io_c] : Yv[(size_t)(r - 2) * nstate + sb + io_c]);
          io[r * ROP_LD + io_c] = v;
        }
        wave_lds_sync();
      }
      const double T = io[c], P = io[ROP_LD + c];
      double yk[NCH];
      double syw = 0.0;
#pragma unroll
      for (int j = 0; j < NCH; ++j) {
        const int k = lane + WAVE * j;
        yk[j] = k < KK ? io[(2 + k) * ROP_LD + c] : 0.0;
        syw = fma(yk[j], rw[j], syw);
      }
      const double sumYW = wave_sum(syw);
      const double rho = P / (RU * T * sumYW);
      const double lnT = log(T), invT = 1.0 / T, lnPRT = LN_PATM_RU - lnT;
      double cpm = 0.0, hm = 0.0;
#pragma unroll
      for (int j = 0; j < NCH; ++j) {
        const int k = lane + WAVE * j;
        if (k < KK) {
          const Thermo7 th = nasa7_img(V, k, T, lnT, invT);
          C[k] = rho * yk[j] * rw[j];
          gRT[k] = th.hRT - th.sR;
          wdot[k] = 0.0;
          cpm += yk[j] * th.cpR * RU * rw[j];
          hm += yk[j] * th.hRT * RU * T * rw[j];
        } else if (k == sp_one) {
          C[sp_one] = 1.0;
          gRT[sp_one] = 0.0;
        }
      }
      const double Ctot = rho * sumYW;
      wave_lds_sync();
      for (int g = lane; g < V.G; g += WAVE) {
        double m = Ctot;
        for (int p = V.gptr()[g]; p < V.gptr()[g + 1]; ++p) m += V.geff()[p] * C[V.gsp()[p]];
        Mg[g] = m;
      }
      wave_lds_sync();
      for (int base = 0; base < V.IIp; base += WAVE) {
        const int i = base + lane;
        const uint32_t inf = V.info()[i];
        const int nr = rx_nr(inf), np = rx_np(inf);
        if constexpr (PL) {
          if (inf & RX_GEN) {  // FORD / RORD / non-integral coefficients
            const double* g;
            const Rxn e = eval_gen_img(V, i, inf, T, lnT, invT, lnPRT, P, C, gRT, gRT, Mg, false, -1, 0.0, 1.0, g);
            const double qf = e.mfac * e.kf * e.pf, qr = e.mfac * e.kr * e.pr;
            if (MODE == 1) {
              const int oi = orig[i];
              o0[(size_t)oi * nstate + st] = qf;
              o1[(size_t)oi * nstate + st] = qr;
            } else {
              const double q = qf - qr;
              for (int u = 0; u < (int)g[0]; ++u) atomicAdd(&wdot[(int)g[2 + 3 * u]], -g[3 + 3 * u] * q);
              for (int u = 0; u < (int)g[1]; ++u) atomicAdd(&wdot[(int)g[GEN_P + 3 * u]], g[GEN_P + 1 + 3 * u] * q);
            }
            continue;
          }
        }
        if (nr + np == 0) continue;
        const uint32_t rs = V.rsp()[i], ps = V.psp()[i];
        const Rxn e = eval_rxn_img<PL>(V, i, inf, rs, ps, 0u, T, lnT, invT, lnPRT, P, C, gRT, gRT, Mg, false);
        const double qf = e.mfac * e.kf * e.pf, qr = e.mfac * e.kr * e.pr;
        if (MODE == 1) {
          const int oi = orig[i];
          o0[(size_t)oi * nstate + st] = qf;
          o1[(size_t)oi * nstate + st] = qr;
        } else {
          const double q = qf - qr;
          const bool s23 = __ballot(nr > 2 || np > 2) != 0;
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            if (u >= 2 && !s23) break;
            if (u < nr) atomicAdd(&wdot[sp_of(rs, u)], -q);
            if (u < np) atomicAdd(&wdot[sp_of(ps, u)], q);
          }
        }
      }
      if (MODE == 0) {
        wave_lds_sync();
#pragma unroll
        for (int j = 0; j < NCH; ++j) {
          const int k = lane + WAVE * j;
          if (k < KK) io[(2 + k) * ROP_LD + c] = wdot[k];
        }
        const double cps = wave_sum(cpm), hs = wave_sum(hm);
        if (lane == 0) {
          io[c] = cps;
          io[ROP_LD + c] = hs;
        }
      }
      wave_lds_sync();  // the next state overwrites C / gRT / wdot
      if (MODE == 0 && (c == cnt - 1)) {
        for (int r = io_r; r < nrow; r += WAVE / ROP_SUB) {
          if (io_c < cnt) {
            const double v = io[r * ROP_LD + io_c];
            if (r >= 2) o0[(size_t)(r - 2) * nstate + sb + io_c] = v;
            else if (r == 0 && o1) o1[sb + io_c] = v;
            else if (r == 1 && o2) o2[sb + io_c] = v;
          }
        }
        wave_lds_sync();  // the next half-chunk's loads overwrite io
      }
    }
  }
}

// species thermo: one thread per state, coefficients read uniformly
__global__ void species_thermo_kernel(MechDev M, int nstate, const double* __restrict__ Tv, double* __restrict__ cp,
                                      double* __restrict__ h, double* __restrict__ s) {
  const int st = blockIdx.x * blockDim.x + threadIdx.x;
  if (st >= nstate) return;
  const double T = Tv[st], lnT = log(T);
  for (int k = 0; k < M.KK; ++k) {
    const SpThermo th = nasa7(M, k, T, lnT);
    if (cp) cp[(size_t)k * nstate + st] = th.cpR;
    if (h) h[(size_t)k * nstate + st] = th.hRT;
    if (s) s[(size_t)k * nstate + st] = th.sR;
  }
}

}  // namespace

// ====================================================================== host side

namespace {

template <typename T>
int upload(ckmi_mech* m, const std::vector<T>& v, const T** out) {
  void* p = nullptr;
  size_t bytes = std::max<size_t>(v.size() * sizeof(T), 16);
  CKMI_HIP_CHECK(hipMalloc(&p, bytes));
  if (!v.empty()) CKMI_HIP_CHECK(hipMemcpy(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
  m->allocs.push_back(p);
  *out = static_cast<const T*>(p);
  return CKMI_OK;
}

template <int MODE, int NCH, bool PL>
int launch_rop_n(const ckmi_mech* m, int n, const double* T, const double* P, const double* Y, double* o0,
                 double* o1, double* o2, hipStream_t stream) {
  constexpr int NW = rop_waves(NCH);
  const size_t lds = (size_t)m->img.bytes + (size_t)NW * rop_slice_bytes(m->G, m->img.KK, m->img.KKp);
  int ncu = 0, per_cu = 0, lds_max = 0;
  CKMI_HIP_CHECK(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, m->device));
  CKMI_HIP_CHECK(hipDeviceGetAttribute(&lds_max, hipDeviceAttributeMaxSharedMemoryPerMultiprocessor, m->device));
  if (lds > (size_t)lds_max) return set_error(CKMI_ERR_SIZE, "mechanism image + ROP work space exceed the LDS of a CU");
  if (int rc = raise_lds_limit(m->device, (const void*)rop_kernel<MODE, NCH, PL>, lds)) return rc;
  CKMI_HIP_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, rop_kernel<MODE, NCH, PL>, NW * WAVE, lds));
  if (per_cu < 1) return set_error(CKMI_ERR_SIZE, "ROP kernel does not fit on a CU");
  const int tasks = (n + ROP_CHUNK - 1) / ROP_CHUNK;
  const int grid = std::max(1, std::min(ncu * per_cu, (tasks + NW - 1) / NW));
  hipLaunchKernelGGL((rop_kernel<MODE, NCH, PL>), dim3(grid), dim3(NW * WAVE), lds, stream, m->img, m->d_orig, n, T, P,
                     Y, o0, o1, o2);
  CKMI_HIP_CHECK(hipGetLastError());
  return CKMI_OK;
}

template <int MODE>
int launch_rop(const ckmi_mech* m, int n, const double* T, const double* P, const double* Y, double* o0, double* o1,
               double* o2, hipStream_t stream) {
  const bool pl = m->has_plog;
  switch (m->img.KKp / WAVE) {
    case 1: return pl ? launch_rop_n<MODE, 1, true>(m, n, T, P, Y, o0, o1, o2, stream)
                      : launch_rop_n<MODE, 1, false>(m, n, T, P, Y, o0, o1, o2, stream);
    case 2: return pl ? launch_rop_n<MODE, 2, true>(m, n, T, P, Y, o0, o1, o2, stream)
                      : launch_rop_n<MODE, 2, false>(m, n, T, P, Y, o0, o1, o2, stream);
    case 3: return pl ? launch_rop_n<MODE, 3, true>(m, n, T, P, Y, o0, o1, o2, stream)
                      : launch_rop_n<MODE, 3, false>(m, n, T, P, Y, o0, o1, o2, stream);
    case 4: return pl ? launch_rop_n<MODE, 4, true>(m, n, T, P, Y, o0, o1, o2, stream)
                      : launch_rop_n<MODE, 4, false>(m, n, T, P, Y, o0, o1, o2, stream);
    default: return set_error(CKMI_ERR_UNSUPPORTED, "mechanism image with more than 255 species");
  }
}

// Makes m's device current for the scope and restores the caller's device afterwards: the
// specialised kernel's module belongs to the device it was loaded on.
struct DeviceScope {
  int prev = -1;
  explicit DeviceScope(int dev) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    if (prev != dev) (void)hipSetDevice(dev);
  }
  ~DeviceScope() {
    int cur = -1;
    if (prev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev) (void)hipSetDevice(prev);
  }
};

// compile and load the specialised ROP kernel of m once (thread-safe), on m's device; CKMI_OK when
// it can run
int jit_ready(ckmi_mech* m) {
  if (!m->jit) return set_error(CKMI_ERR_UNSUPPORTED, "no specialised ROP kernel");
  JitRop& J = *m->jit;
  if (J.state.load() == 1) return CKMI_OK;
  std::lock_guard<std::mutex> lk(J.mu);
  if (J.state.load() == 1) return CKMI_OK;
  if (J.state.load() == -1) return set_error(CKMI_ERR_UNSUPPORTED, "specialised ROP kernel unavailable: " + J.why);
  std::vector<char> code;
  std::string log;
  const int rc = jit_rop_compile(J.src, code, log);
  if (rc) {
    J.why = "hipRTC compilation failed: " + log.substr(0, 2000);
    J.state.store(-1);
    return set_error(CKMI_ERR_HIP, J.why);
  }
  DeviceScope on(m->device);
  if (hipModuleLoadData(&J.mod, code.data()) != hipSuccess ||
      hipModuleGetFunction(&J.fn, J.mod, ("ckjit_rop_k" + std::to_string(m->KK) + "_i" + std::to_string(m->II)).c_str()) !=
          hipSuccess) {
    J.why = "hipModuleLoadData / hipModuleGetFunction failed";
    J.state.store(-1);
    return set_error(CKMI_ERR_HIP, J.why);
  }
  J.state.store(1);
  return CKMI_OK;
}

}  // namespace

int ckmi::set_error(int code, const std::string& msg) {
  g_err = msg;
  return code;
}

// ---------------------------------------------------------------- the launch layer (ckmi_internal.hpp)
int ckmi::stage_cfg(const DevCfg& dc, DevCfg* dst, hipStream_t stream) {
  auto* hc = new DevCfg(dc);
  const hipError_t e = hipMemcpyAsync(dst, hc, sizeof(DevCfg), hipMemcpyHostToDevice, stream);
  if (e != hipSuccess) {
    delete hc;
    return set_error(CKMI_ERR_HIP, std::string("cfg copy: ") + hipGetErrorString(e));
  }
  CKMI_HIP_CHECK(hipLaunchHostFunc(stream, [](void* p) { delete static_cast<DevCfg*>(p); }, hc));
  return CKMI_OK;
}

int ckmi::raise_lds_limit(int device, const void* fn, size_t bytes) {
  if (bytes <= 64 * 1024) return CKMI_OK;
  static thread_local std::map<std::pair<int, const void*>, size_t> limit;
  size_t& set = limit[{device, fn}];
  if (set < bytes) {
    CKMI_HIP_CHECK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    set = bytes;
  }
  return CKMI_OK;
}

DevCfg ckmi::make_dev_cfg(const ckmi_mech* m, const ckmi_reactor_cfg* cfg, bool integrate) {
  DevCfg dc;  // the call's own configuration (staged per launch: no state shared between calls)
  dc.c = *cfg;
  if (dc.c.gfac == 0.0) dc.c.gfac = 1.0;
  dc.ncrit = 0;
  if (integrate) {  // the sorted union of the profiles' breakpoints in (0, t_end)
    std::vector<double> tc;
    for (int i = 0; i < cfg->nprof; ++i)
      if (cfg->prof_t[i] > 0.0 && cfg->prof_t[i] < cfg->t_end) tc.push_back(cfg->prof_t[i]);
    for (int i = 0; i < cfg->nprof2; ++i)
      if (cfg->prof2_t[i] > 0.0 && cfg->prof2_t[i] < cfg->t_end) tc.push_back(cfg->prof2_t[i]);
    for (int i = 0; i < cfg->nprof3; ++i)
      if (cfg->prof3_t[i] > 0.0 && cfg->prof3_t[i] < cfg->t_end) tc.push_back(cfg->prof3_t[i]);
    std::sort(tc.begin(), tc.end());
    tc.erase(std::unique(tc.begin(), tc.end()), tc.end());
    dc.ncrit = (int)tc.size();
    std::copy(tc.begin(), tc.end(), dc.tcrit);
  }
  dc.guard_y = std::max(1e-3, 1e3 * cfg->atol);
  dc.guard_tlo = m->tguard_lo;
  dc.guard_thi = m->tguard_hi;
  dc.npe = (integrate && !cfg->no_elem_proj) ? m->npe : 0;
  return dc;
}

int ckmi::check_reactor_cfg(const ckmi_reactor_cfg* cfg, const ckmi_reactor_ext* ext, bool profiles) {
  if (cfg->energy != 1 && cfg->energy != 2) return set_error(CKMI_ERR_ARG, "energy must be 1 or 2");
  if (!(cfg->gfac >= 0.0)) return set_error(CKMI_ERR_ARG, "GFAC must be >= 0");
  if (!(cfg->htc >= 0.0) || !(cfg->areaq >= 0.0) || !(cfg->tamb > 0.0 || cfg->htc * cfg->areaq == 0.0))
    return set_error(CKMI_ERR_ARG, "HTC, AREAQ must be >= 0 and TAMB > 0");
  if (ext && (ext->afac_rxn != nullptr) != (ext->afac != nullptr))
    return set_error(CKMI_ERR_ARG, "afac_rxn and afac go together");
  if (!profiles) return CKMI_OK;
  if (cfg->nprof < 0 || cfg->nprof > 64) return set_error(CKMI_ERR_ARG, "nprof must be in [0, 64]");
  if (cfg->nprof2 < 0 || cfg->nprof2 > 64) return set_error(CKMI_ERR_ARG, "nprof2 must be in [0, 64]");
  if (cfg->nprof3 < 0 || cfg->nprof3 > 64) return set_error(CKMI_ERR_ARG, "nprof3 must be in [0, 64]");
  if (cfg->prof_kind != 0 && cfg->prof_kind != 1)
    return set_error(CKMI_ERR_ARG, "prof_kind must be 0 (VPRO/PPRO) or 1 (TPRO)");
  if (cfg->prof_kind == 1 && cfg->energy != 2)
    return set_error(CKMI_ERR_ARG, "TPRO needs a given-temperature run (energy = 2)");
  if (cfg->nprof2 > 0 && cfg->prof2_kind != 1 && cfg->prof2_kind != 2)
    return set_error(CKMI_ERR_ARG, "prof2_kind must be 1 (QPRO) or 2 (AEXT)");
  if (cfg->nprof2 > 0 && cfg->energy != 1) return set_error(CKMI_ERR_ARG, "QPRO / AEXT need an energy-equation run");
  if (cfg->nprof3 > 0 && !(cfg->nprof2 > 0 && cfg->prof2_kind == 1))
    return set_error(CKMI_ERR_ARG, "the third profile (AEXT) needs a QPRO second profile");
  return CKMI_OK;
}

namespace {
// ckmi_mech_create on a fresh handle: build on the host (ckmi_mech_host.cpp), upload, set up the specialised
// ROP kernel.  The caller destroys the handle when this fails.
int mech_create(const ckmi_mech_desc* d, ckmi_mech* m) {
  const char* lanes = std::getenv("CKMI_LANES");  // A/B knob: CKMI_LANES=0 keeps the file order
  if (int rc = build_host_mech(d, !(lanes && lanes[0] == '0'), *m)) return rc;
  if (hipGetDevice(&m->device) != hipSuccess) return set_error(CKMI_ERR_HIP, "no HIP device");
  m->d.KK = m->KK;
  const char* blob = nullptr;
  int rc = upload(m, m->wt, &m->d.wt);
  if (!rc) rc = upload(m, m->rwt, &m->d.rwt);
  if (!rc) rc = upload(m, m->th, &m->d.th);
  if (!rc) rc = upload(m, m->orig, &m->d_orig);
  if (!rc) rc = upload(m, m->slot_of, &m->img.slot_of);
  if (!rc) rc = upload(m, m->jcol_ptr, &m->img.jcol_ptr);
  if (!rc) rc = upload(m, m->jcol_ent, &m->img.jcol_ent);
  if (!rc) rc = upload(m, m->blob, &blob);
  if (rc) return rc;
  m->img.blob = (const uint4*)blob;
  std::vector<char>().swap(m->blob);  // the device copy is the image from here on (ckmi_set_afactor edits it)
  // the mechanism-specialised ROP kernel: source and parameter block now, compilation at first use
  m->jit = new JitRop();
  {
    std::vector<double> prm;
    const char* env = std::getenv("CKMI_ROP_JIT");
    if (env && env[0] == '0') {
      m->jit->state = -1;
      m->jit->why = "disabled by CKMI_ROP_JIT=0";
    } else if (!jit_rop_generate(d, m->jit->src, prm, m->jit->lnA_off, m->jit->why)) {
      m->jit->state = -1;
    } else {
      const double* p = nullptr;
      if (int rc = upload(m, prm, &p)) return rc;
      m->jit->prm = const_cast<double*>(p);
      if (const char* dump = std::getenv("CKMI_JIT_DUMP")) {
        if (FILE* f = std::fopen(dump, "w")) {
          std::fputs(m->jit->src.c_str(), f);
          std::fclose(f);
        }
      }
    }
  }
  return CKMI_OK;
}
}  // namespace

extern "C" {

const char* ckmi_last_error(void) { return g_err.c_str(); }

#ifdef CKMI_PHASE_TIMERS
// diagnostic build only: buf = device u64 [n][8] (rhs, jac, lu, solve, total cycles)
int ckmi_debug_phase_buffer(void* buf) {
  CKMI_HIP_CHECK(hipMemcpyToSymbol(HIP_SYMBOL(g_phase_buf), &buf, sizeof(buf)));
  return CKMI_OK;
}
#endif
int ckmi_version(void) { return CKMI_ABI_VERSION; }

int ckmi_mech_create(const ckmi_mech_desc* d, ckmi_mech** out) {
  if (!d || !out) return set_error(CKMI_ERR_ARG, "null argument");
  auto* m = new ckmi_mech();
  const int rc = mech_create(d, m);
  if (rc) ckmi_mech_destroy(m);  // the one way out of a failed create: frees what was uploaded so far
  else *out = m;
  return rc;
}

int ckmi_mech_destroy(ckmi_mech* m) {
  if (!m) return CKMI_OK;
  if (m->jit) {
    if (m->jit->mod) (void)hipModuleUnload(m->jit->mod);
    delete m->jit;
  }
  for (void* p : m->allocs) (void)hipFree(p);
  delete m;
  return CKMI_OK;
}

int ckmi_mech_sizes(const ckmi_mech* m, int32_t* KK, int32_t* II) {
  if (!m) return set_error(CKMI_ERR_ARG, "null mech");
  if (KK) *KK = m->KK;
  if (II) *II = m->II;
  return CKMI_OK;
}

int ckmi_get_arrhenius(const ckmi_mech* m, double* A, double* b, double* E) {
  if (!m) return set_error(CKMI_ERR_ARG, "null mech");
  for (int i = 0; i < m->II; ++i) {
    if (A) A[i] = std::exp(m->lnA_orig[i]);
    if (b) b[i] = m->b_orig[i];
    if (E) E[i] = m->E_orig[i];
  }
  return CKMI_OK;
}

int ckmi_reaction_slots(const ckmi_mech* m, int32_t* slot) {
  if (!m || !slot) return set_error(CKMI_ERR_ARG, "null mech or slot array");
  for (int i = 0; i < m->II; ++i) slot[i] = m->slot_of[i];
  return CKMI_OK;
}

int ckmi_set_afactor(ckmi_mech* m, int32_t irxn, double A) {
  if (!m || irxn < 0 || irxn >= m->II || !(A > 0.0)) return set_error(CKMI_ERR_ARG, "bad reaction index or A");
  if (m->rtype_orig[irxn] == CKMI_RXN_PLOG || m->rtype_orig[irxn] == CKMI_RXN_CHEB)
    return set_error(CKMI_ERR_UNSUPPORTED, "A-factor of a PLOG / Chebyshev reaction (its rate comes from its table)");
  const double lnA = std::log(A);
  m->lnA_orig[irxn] = lnA;
  const int s = m->slot_of[irxn];
  CKMI_HIP_CHECK(hipMemcpy((char*)m->img.blob + m->img.o_lnA + sizeof(double) * s, &lnA, sizeof(double),
                      hipMemcpyHostToDevice));
  if (m->jit && m->jit->prm) {
    CKMI_HIP_CHECK(hipMemcpy(m->jit->prm + m->jit->lnA_off[irxn], &lnA, sizeof(double), hipMemcpyHostToDevice));
    if (m->b_orig[irxn] == 0.0 && m->E_orig[irxn] == 0.0)  // k = A reactions read A itself (ckmi_jit.cpp)
      CKMI_HIP_CHECK(hipMemcpy(m->jit->prm + m->jit->lnA_off[irxn] + 1, &A, sizeof(double), hipMemcpyHostToDevice));
  }
  return CKMI_OK;
}

int ckmi_species_thermo(const ckmi_mech* m, int32_t n, const double* T, double* cp_R, double* h_RT, double* s_R,
                        void* stream) {
  if (!m || n < 0) return set_error(CKMI_ERR_ARG, "bad argument");
  if (n == 0) return CKMI_OK;
  const int bs = 256;
  hipLaunchKernelGGL(species_thermo_kernel, dim3((n + bs - 1) / bs), dim3(bs), 0, (hipStream_t)stream, m->d, n, T, cp_R,
                     h_RT, s_R);
  CKMI_HIP_CHECK(hipGetLastError());
  return CKMI_OK;
}

int ckmi_rop_thermo(const ckmi_mech* m, int32_t n, const double* T, const double* P, const double* Y, double* wdot,
                    double* cp, double* h, void* stream) {
  if (!m || n < 0 || !wdot) return set_error(CKMI_ERR_ARG, "bad argument");
  if (n == 0) return CKMI_OK;
  const int path = g_rop_path.load();
  if (path == 2 || (path == 0 && n >= JIT_MIN_STATES)) {
    const int rc = jit_ready(const_cast<ckmi_mech*>(m));
    if (rc == CKMI_OK) {
      DeviceScope on(m->device);
      void* args[] = {&n, (void*)&T, (void*)&P, (void*)&Y, &wdot, &cp, &h, &m->jit->prm};
      CKMI_HIP_CHECK(hipModuleLaunchKernel(m->jit->fn, (unsigned)((n + 63) / 64), 1, 1, 64, 1, 1, 0, (hipStream_t)stream,
                                      args, nullptr));
      return CKMI_OK;
    }
    if (path == 2) return rc;
  }
  return launch_rop<0>(m, n, T, P, Y, wdot, cp, h, (hipStream_t)stream);
}

int ckmi_set_rop_path(int32_t path) {
  if (path < 0 || path > 2) return set_error(CKMI_ERR_ARG, "rop path must be 0 (auto), 1 (generic) or 2 (specialised)");
  g_rop_path = path;
  return CKMI_OK;
}

int ckmi_rop_jit_source(const ckmi_mech_desc* d, char* buf, int64_t cap, int64_t* len) {
  if (!d || !len) return set_error(CKMI_ERR_ARG, "null argument");
  std::string src, why;
  std::vector<double> prm;
  std::vector<int> off;
  if (!jit_rop_generate(d, src, prm, off, why)) return set_error(CKMI_ERR_UNSUPPORTED, why);
  *len = (int64_t)src.size();
  if (buf && cap > 0) {
    const size_t k = std::min<size_t>((size_t)cap - 1, src.size());
    std::memcpy(buf, src.data(), k);
    buf[k] = 0;
  }
  return CKMI_OK;
}

int ckmi_rop_jit_compile(const ckmi_mech_desc* d, int64_t* code_bytes) {
  if (!d || !code_bytes) return set_error(CKMI_ERR_ARG, "null argument");
  std::string src, why, log;
  std::vector<double> prm;
  std::vector<int> off;
  if (!jit_rop_generate(d, src, prm, off, why)) return set_error(CKMI_ERR_UNSUPPORTED, why);
  std::vector<char> code;
  if (jit_rop_compile(src, code, log)) return set_error(CKMI_ERR_HIP, "hipRTC compilation failed: " + log.substr(0, 2000));
  *code_bytes = (int64_t)code.size();
  return CKMI_OK;
}

int ckmi_rop_jit_state(const ckmi_mech* m, int32_t* state) {
  if (!m || !state) return set_error(CKMI_ERR_ARG, "null argument");
  *state = m->jit ? m->jit->state.load() : -1;
  if (*state == -1 && m->jit) {
    std::lock_guard<std::mutex> lk(m->jit->mu);
    g_err = m->jit->why;
  }
  return CKMI_OK;
}

int ckmi_reaction_rates(const ckmi_mech* m, int32_t n, const double* T, const double* P, const double* Y, double* qf,
                        double* qr, void* stream) {
  if (!m || n < 0 || !qf || !qr) return set_error(CKMI_ERR_ARG, "bad argument");
  if (n == 0) return CKMI_OK;
  return launch_rop<1>(m, n, T, P, Y, qf, qr, nullptr, (hipStream_t)stream);
}

namespace {
// The closed-reactor instantiations, named in the order the code object has always held them.  Kernels are laid
// out in the order they are first named; it is fixed here, not left to the order the chooser's visitor happens to
// name them in, so that a change to the host code leaves the device code object byte for byte as it was (which is
// how such a change is checked: profiles/launch_layer_kernel_resources.txt).
#ifndef CKMI_PROBE_C3
[[maybe_unused]] constexpr int (*REACTOR_VARIANTS[])(const ckmi_mech*, int, const DevCfg&, const ReactorIO&, hipStream_t,
                                                      int) = {
    launch_reactors<64, true, true>, launch_reactors<64, true, false>,  launch_reactors<54, false, true>,
    launch_reactors<32>,             launch_reactors<54, false, false>, launch_reactors<64, false, true>,
    launch_reactors<64, false, false>};
#endif
}  // namespace

int ckmi_reactor_run_ex(const ckmi_mech* m, const ckmi_reactor_cfg* cfg, int32_t n, const int32_t* problem,
                        const double* T0, const double* P0, const double* V0, const double* Y0,
                        const ckmi_reactor_ext* ext, double* tau, double* Tend, double* Pend, double* Vend,
                        double* Yend, int32_t* stats, int32_t nsave, const double* t_save, double* y_save,
                        void* stream) {
  if (!m || !cfg || n < 0) return set_error(CKMI_ERR_ARG, "bad argument");
  if (int rc = check_reactor_cfg(cfg, ext, true)) return rc;
  if (!(cfg->t_end > 0.0) || !(cfg->rtol > 0.0) || !(cfg->atol > 0.0)) return set_error(CKMI_ERR_ARG, "t_end, rtol, atol must be > 0");
  if (cfg->ign_mode < 0 || cfg->ign_mode > 4) return set_error(CKMI_ERR_ARG, "bad ignition mode");
  if (cfg->ign_mode == 4 && (cfg->ign_species < 0 || cfg->ign_species >= m->KK)) return set_error(CKMI_ERR_ARG, "bad KLIM species");
  if (cfg->asteps < 0) return set_error(CKMI_ERR_ARG, "asteps must be >= 0");
  if (nsave > 0 && (!t_save || !y_save)) return set_error(CKMI_ERR_ARG, "t_save / y_save required when nsave > 0");
  if (ext && ext->n_adap && (ext->max_adap <= 0 || !ext->t_adap || !ext->y_adap))
    return set_error(CKMI_ERR_ARG, "n_adap needs max_adap > 0, t_adap and y_adap");
  if (cfg->avar > m->KK || cfg->avar < -1) return set_error(CKMI_ERR_ARG, "avar must be -1, 0 (T) or 1 + species index");
  if (cfg->eng[CKMI_ENG_HTMODEL] == 1.0 && !cfg->tran)
    return set_error(CKMI_ERR_ARG, "the engine's ICHX heat transfer needs the transport fits (cfg->tran)");
  if (n == 0) return CKMI_OK;
  const DevCfg dc = make_dev_cfg(m, cfg, true);
  ReactorIO io{problem, T0, P0, V0, Y0, tau, Tend, Pend, Vend, Yend, stats, nsave, t_save, y_save,
               ext ? ext->afac_rxn : nullptr, ext ? ext->afac : nullptr, ext ? ext->max_adap : 0,
               ext ? ext->t_adap : nullptr, ext ? ext->y_adap : nullptr, ext ? ext->n_adap : nullptr,
               ext ? ext->t_stop : nullptr};
  const int nvar = m->KK + 1;
  const int rpath = g_reactor_path.load();
  const hipStream_t st = (hipStream_t)stream;
  int rc = CKMI_OK;
  // more than 63 species: one workgroup per reactor (ckmi_big.hip); else one wave per reactor
  if (use_workgroup_kernel(nvar, rpath)) {
    // the workgroup kernel has no engine model: checked on the host (one synchronous copy of problem[])
    std::vector<int32_t> hp(n);
    CKMI_HIP_CHECK(hipMemcpyAsync(hp.data(), problem, sizeof(int32_t) * n, hipMemcpyDeviceToHost, st));
    CKMI_HIP_CHECK(hipStreamSynchronize(st));
    if (std::find(hp.begin(), hp.end(), 4) != hp.end())
      return set_error(CKMI_ERR_UNSUPPORTED, "engine reactors (problem 4) need KK + 1 <= 64 (the wave-per-reactor kernel)");
    rc = launch_big_reactors(m, n, dc, io, st);
  } else {
    // An FP32-inverse launch skips the plug-flow reactors and an FP64-inverse launch of the same size
    // follows it for them (it pulls and drops the other indices: ~0.1 ms per 65,536 reactors when
    // there are none); the problem array is device memory, so the host cannot tell in advance.
    const WavePlan p = wave_plan(nvar, m->has_plog, m->has_general, cfg->rtol, rpath, false);
    if (p.n32)
      rc = visit_wave_variant<false>(p.n32, p.pl, [&](auto N, auto PL) {
        return launch_reactors<decltype(N)::value, decltype(PL)::value, false>(m, n, dc, io, st, SEL_NO_PFR);
      });
    if (!rc)
      rc = visit_wave_variant<true>(p.n64, p.pl, [&](auto N, auto PL) {
        return launch_reactors<decltype(N)::value, decltype(PL)::value, true>(m, n, dc, io, st, f64_sel(p.f64_takes));
      });
  }
  if (rc) return rc;
  CKMI_HIP_CHECK(hipGetLastError());
  return CKMI_OK;
}

int ckmi_engine_heat_rates(const ckmi_mech* m, const ckmi_reactor_cfg* cfg, double T0, double P0, const double* Y0,
                           int32_t n, const double* t, const double* y, double* ahrr, double* qloss, void* stream) {
  if (!m || !cfg || n < 0 || !Y0 || (n > 0 && (!t || !y || !ahrr || !qloss))) return set_error(CKMI_ERR_ARG, "bad argument");
  if (!(T0 > 0.0) || !(P0 > 0.0)) return set_error(CKMI_ERR_ARG, "T0 and P0 must be > 0");
  if (m->KK + 1 > WAVE) return set_error(CKMI_ERR_UNSUPPORTED, "engine heat rates need KK + 1 <= 64 (as engine runs)");
  if (cfg->eng[CKMI_ENG_HTMODEL] == 1.0 && !cfg->tran)
    return set_error(CKMI_ERR_ARG, "the engine's ICHX heat transfer needs the transport fits (cfg->tran)");
  if (n == 0) return CKMI_OK;
  const DevCfg dc = make_dev_cfg(m, cfg, false);
  const hipStream_t st = (hipStream_t)stream;
  const size_t lds = (size_t)align16(m->img.bytes) + slice_vec_bytes(m->G) + align16((int)sizeof(RunCtx));
  const void* fn = m->has_plog ? (const void*)engine_heat_kernel<true> : (const void*)engine_heat_kernel<false>;
  if (int rc = raise_lds_limit(m->device, fn, lds)) return rc;
  const size_t cbytes = StreamWorkspace::aligned(sizeof(DevCfg));
  StreamWorkspace ws(st);
  if (int rc = ws.alloc(cbytes)) return rc;
  DevCfg* dcfg = ws.take<DevCfg>(cbytes);
  if (int rc = stage_cfg(dc, dcfg, st)) return rc;
  const int grid = std::min(n, 4096);
  if (m->has_plog)
    hipLaunchKernelGGL(engine_heat_kernel<true>, dim3(grid), dim3(WAVE), lds, st, m->img, (const DevCfg*)dcfg, T0, P0,
                       Y0, n, t, y, ahrr, qloss);
  else
    hipLaunchKernelGGL(engine_heat_kernel<false>, dim3(grid), dim3(WAVE), lds, st, m->img, (const DevCfg*)dcfg, T0, P0,
                       Y0, n, t, y, ahrr, qloss);
  CKMI_HIP_CHECK(hipGetLastError());
  return CKMI_OK;
}

int ckmi_reactor_rhs_jac(const ckmi_mech* m, const ckmi_reactor_cfg* cfg, int32_t n, const int32_t* problem,
                         const double* T0, const double* P0, const double* V0, const double* Y0, const double* t,
                         const double* y, const ckmi_reactor_ext* ext, const ckmi_rhs_psr* psr, double* f, double* J,
                         void* stream) {
  if (!m || !cfg || n < 0) return set_error(CKMI_ERR_ARG, "bad argument");
  if (n > 0 && (!problem || !T0 || !P0 || !V0 || !Y0 || !t || !y || !f))
    return set_error(CKMI_ERR_ARG, "problem, T0, P0, V0, Y0, t, y and f are required");
  if (int rc = check_reactor_cfg(cfg, ext, true)) return rc;
  if (n == 0) return CKMI_OK;
  const hipStream_t st = (hipStream_t)stream;
  // the problems decide the kernel: checked on the host (one synchronous copy; a diagnostic call)
  std::vector<int32_t> hp(n);
  CKMI_HIP_CHECK(hipMemcpyAsync(hp.data(), problem, sizeof(int32_t) * n, hipMemcpyDeviceToHost, st));
  CKMI_HIP_CHECK(hipStreamSynchronize(st));
  int n_lo = 0, n_pf = 0, n_eng = 0, n_psr = 0;
  for (int32_t p : hp) {
    if (p < 1 || p > 5) return set_error(CKMI_ERR_ARG, "problem must be 1..5 for every state");
    n_lo += p <= 2, n_pf += p == 3, n_eng += p == 4, n_psr += p == 5;
  }
  if (n_psr && n_psr != n) return set_error(CKMI_ERR_ARG, "open reactors (problem 5) cannot share a call with closed ones");
  const int nvar = m->KK + 1;
  const int rpath = g_reactor_path.load();
  if ((n_eng || n_psr) && nvar > WAVE_NMAX)
    return set_error(CKMI_ERR_UNSUPPORTED, "engine and open reactors (problems 4, 5) need KK + 1 <= 64");
  if (n_eng && rpath == 1)
    return set_error(CKMI_ERR_UNSUPPORTED, "engine reactors (problem 4) need the wave-per-reactor kernel");
  if (n_eng && cfg->eng[CKMI_ENG_HTMODEL] == 1.0 && !cfg->tran)
    return set_error(CKMI_ERR_ARG, "the engine's ICHX heat transfer needs the transport fits (cfg->tran)");
  if (n_psr) {
    if (!psr || (psr->mode != 1 && psr->mode != 2) || !psr->Tin || !psr->Yin || !psr->mdot)
      return set_error(CKMI_ERR_ARG, "problem 5 needs the inlet block: mode 1 or 2, Tin, Yin, mdot");
    if (cfg->nprof != 0 || cfg->nprof2 != 0 || cfg->nprof3 != 0) return set_error(CKMI_ERR_ARG, "profiles do not apply to a PSR");
  }
  const DevCfg dc = make_dev_cfg(m, cfg, false);
  ProbeIO io{problem, T0, P0, V0, Y0, t, y, ext ? ext->afac_rxn : nullptr, ext ? ext->afac : nullptr,
             psr ? psr->Tin : nullptr, psr ? psr->Yin : nullptr, psr ? psr->mdot : nullptr, psr ? psr->mode : 0, f, J};
  if (n_psr) return launch_psr_probe(m, n, dc, io, st);
  if (use_workgroup_kernel(nvar, rpath)) return launch_big_probe(m, n, dc, io, st);
  // the plan of ckmi_reactor_run_ex: problems 1 and 2 in the FP32-inverse variant (PF = false) unless the FP64
  // inverse is selected, plug flow and engines in the FP64-inverse one (PF = true); a launch with no state is left out
  const WavePlan p = wave_plan(nvar, m->has_plog, m->has_general, cfg->rtol, rpath, false);
  const int sel = p.f64_takes == F64_TAKES_ALL ? SEL_ALL : SEL_PFR;  // (one evaluation: nothing to take again)
  const auto probe = [&](auto PL) {
    int rc = CKMI_OK;
    if (p.n32 && n_lo) rc = launch_rhs_probe<decltype(PL)::value, false, false>(m, n, dc, io, SEL_NO_PFR, p.n32, st);
    if (!rc && (!p.n32 || n_pf + n_eng)) rc = launch_rhs_probe<decltype(PL)::value, true, false>(m, n, dc, io, sel, p.n64, st);
    return rc;
  };
  return p.pl ? probe(std::true_type{}) : probe(std::false_type{});
}

int ckmi_newton_probe(int32_t kernel, int32_t size, int32_t f32_stored, int32_t nsys, int32_t n, const float* J,
                      const double* gamma, const float* J_prev, const double* gamma_prev, int32_t nrhs, const double* B,
                      double b_pad, double* X, int32_t* perm, int32_t* ok, void* stream) {
  if (kernel != 1 && kernel != 2) return set_error(CKMI_ERR_ARG, "kernel must be 1 (wave) or 2 (workgroup)");
  if (nsys < 0 || nrhs < 0) return set_error(CKMI_ERR_ARG, "nsys and nrhs must be >= 0");
  if (f32_stored != 0 && f32_stored != 1) return set_error(CKMI_ERR_ARG, "f32_stored must be 0 or 1");
  if (kernel == 2 && (f32_stored || b_pad != 0.0))
    return set_error(CKMI_ERR_ARG, "the workgroup kernel's matrix has no FP32-stored form, and its solve takes b = 0 beyond n");
  // the sizes the choosers' visitors compile (a size they do not know is refused below, by the visitor itself)
  const int nmax = kernel == 1 ? size : 16 * size;
  if (size < 1 || size > BIG_NMAX || n < 2 || n > nmax) return set_error(CKMI_ERR_ARG, "n must be in [2, the variant's size]");
  if (nsys > 0 && (!J || !gamma || !perm || !ok || (nrhs > 0 && (!B || !X))))
    return set_error(CKMI_ERR_ARG, "J, gamma, perm and ok are required, and B and X with nrhs > 0");
  if ((J_prev == nullptr) != (gamma_prev == nullptr)) return set_error(CKMI_ERR_ARG, "J_prev and gamma_prev go together");
  const NewtonProbeIO io{nsys, n, nrhs, J, J_prev, gamma, gamma_prev, B, b_pad, X, perm, ok};
  const hipStream_t st = (hipStream_t)stream;
  if (kernel == 2) {
    if (size < 4 || size > 12) return set_error(CKMI_ERR_ARG, "the workgroup kernel is compiled for NB = 4..12");
    return nsys == 0 ? CKMI_OK : launch_big_newton_probe(size, io, st);
  }
  const auto probe = [&](auto F64) {
    return visit_wave_variant<decltype(F64)::value>(size, false, [&](auto N, auto) {
      return nsys == 0 ? CKMI_OK : launch_newton_probe<decltype(N)::value, decltype(F64)::value>(io, st);
    });
  };
  return f32_stored ? probe(std::false_type{}) : probe(std::true_type{});
}

int ckmi_reactor_variant(int32_t nvar, int32_t has_plog, int32_t has_general, double rtol, int32_t path,
                         int32_t open_reactor, int32_t out[5]) {
  if (nvar < 2 || path < 0 || path > 3 || !out) return CKMI_ERR_ARG;
  std::fill(out, out + 5, 0);
  if (!open_reactor && use_workgroup_kernel(nvar, path)) {
    const BigPlan p = big_plan(nvar, has_plog != 0);
    if (p.nb == 0) return CKMI_ERR_UNSUPPORTED;
    out[0] = 2, out[1] = p.nb, out[3] = p.pl;
  } else {
    if (nvar > WAVE_NMAX) return CKMI_ERR_UNSUPPORTED;  // open reactors exist in the wave kernel only
    const WavePlan p = wave_plan(nvar, has_plog != 0, has_general != 0, rtol, path, open_reactor != 0);
    out[0] = 1, out[1] = p.n32, out[2] = p.n64, out[3] = p.pl, out[4] = p.f64_takes;
  }
  return CKMI_OK;
}

int ckmi_set_reactor_path(int32_t path) {
  if (path < 0 || path > 3)
    return set_error(CKMI_ERR_ARG, "reactor path must be 0 (automatic), 1 (workgroup), 2 (wave, FP64 inverse) or 3 (wave, "
                              "FP32-stored inverse)");
  g_reactor_path = path;
  return CKMI_OK;
}

int ckmi_reactor_run(const ckmi_mech* m, const ckmi_reactor_cfg* cfg, int32_t n, const int32_t* problem,
                     const double* T0, const double* P0, const double* V0, const double* Y0, double* tau, double* Tend,
                     double* Pend, double* Vend, double* Yend, int32_t* stats, int32_t nsave, const double* t_save,
                     double* y_save, void* stream) {
  return ckmi_reactor_run_ex(m, cfg, n, problem, T0, P0, V0, Y0, nullptr, tau, Tend, Pend, Vend, Yend, stats, nsave,
                             t_save, y_save, stream);
}

}  // extern "C"
