// ckmi.hip -- gfx950 kernels and the C ABI of libckmi.so (see include/ckmi.h).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
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

// ---------------------------------------------------------------- LDS lane assignment
// The reaction strips scatter each lane's rate into the wave's wdot[] with one LDS atomic per unit
// slot (reactor_rhs, rop_kernel) and gather C[] / g/RT[] through the same slots.  Which reaction sits
// on which lane of its (type, slot-class) block, and in which order a reaction's unit slots are
// listed, are free choices (products and sums over the slots commute); they decide the LDS bank
// conflicts: ds_add_f64 is serviced in 16-lane groups on banks (a/4) mod 32, so two lanes of a group
// adding to one species (or to species k and k + 16) serialise; ds_read_b64 in 32-lane groups on
// banks (a/4) mod 64, where distinct species k and k + 32 collide.  Common species (H, O, OH, H2O)
// make the mechanism's file order 4x conflict-bound (GRI-3.0: 456 LDS cycles of atomics per RHS
// against 108 conflict-free, model below).  A deterministic annealing over lane swaps within a block
// and slot orders within a reaction minimises the modelled cycles; the device code is unchanged.
namespace lanes {
struct Rx {
  int ns[2];        // unit slots per side (a species with coefficient c occupies c slots)
  uint8_t sp[2][4]; // the slots' species
};
// modelled LDS cycles of one strip (64 lanes): atomics (16-lane groups, max bank multiplicity) +
// two gathers per slot (32-lane groups, max distinct addresses per bank)
static int strip_cost(const std::vector<Rx>& rx, const std::vector<int>& lane_rx, int s0) {
  bool s23 = false;
  for (int l = 0; l < WAVE; ++l) {
    const int r = lane_rx[s0 + l];
    if (r >= 0 && (rx[r].ns[0] > 2 || rx[r].ns[1] > 2)) s23 = true;
  }
  int cost = 0;
  for (int side = 0; side < 2; ++side)
    for (int u = 0; u < (s23 ? 4 : 2); ++u) {
      for (int g0 = 0; g0 < WAVE; g0 += 16) {  // atomics
        int mult[32] = {0}, mx = 0;
        for (int l = g0; l < g0 + 16; ++l) {
          const int r = lane_rx[s0 + l];
          if (r < 0 || u >= rx[r].ns[side]) continue;
          mx = std::max(mx, ++mult[(2 * rx[r].sp[side][u]) & 31]);
        }
        cost += mx;
      }
      for (int g0 = 0; g0 < WAVE; g0 += 32) {  // gathers (C and g/RT: counted twice)
        int seen[64];
        int nseen = 0, mult[64] = {0}, mx = 0;
        for (int l = g0; l < g0 + 32; ++l) {
          const int r = lane_rx[s0 + l];
          if (r < 0 || u >= rx[r].ns[side]) continue;
          const int k = rx[r].sp[side][u];
          bool dup = false;
          for (int q = 0; q < nseen; ++q) dup |= seen[q] == k;
          if (dup) continue;
          seen[nseen++] = k;
          mx = std::max(mx, ++mult[(2 * k) & 63]);
        }
        cost += 2 * mx;
      }
    }
  return cost;
}
}  // namespace lanes

// slots: device slot -> original reaction (-1 pad), reordered in place within (rtype, slot class)
// blocks; perm[i]: the unit-slot order of original reaction i (reactant slots 0..3, product 4..7)
void assign_lanes(const ckmi_mech_desc* d, std::vector<int>& slots, const std::vector<int>& blk,
                  std::vector<std::array<uint8_t, 8>>& perm) {
  using lanes::Rx;
  const int II = d->II, n = (int)slots.size();
  std::vector<Rx> rx(II);
  perm.assign(II, {0, 1, 2, 3, 0, 1, 2, 3});
  for (int i = 0; i < II; ++i) {
    Rx& r = rx[i];
    for (int side = 0; side < 2; ++side) {
      const int ns = side == 0 ? d->nr[i] : d->np[i];
      const int32_t* sp = (side == 0 ? d->rsp : d->psp) + CKMI_SLOTS * i;
      const double* nu = (side == 0 ? d->rnu : d->pnu) + CKMI_SLOTS * i;
      int c = 0;
      for (int u = 0; u < ns && !rxn_general(d, i); ++u)
        for (int k = 0; k < (int)nu[u] && c < 4; ++k) r.sp[side][c++] = (uint8_t)sp[u];
      r.ns[side] = rxn_general(d, i) ? 0 : c;
    }
  }
  const int nstrip = n / WAVE;
  std::vector<int> cost(nstrip);
  for (int s = 0; s < nstrip; ++s) cost[s] = lanes::strip_cost(rx, slots, s * WAVE);
  uint64_t st = 0x9e3779b97f4a7c15ull;  // deterministic: the same image on every run and device
  auto rnd = [&]() {
    st ^= st << 13, st ^= st >> 7, st ^= st << 17;
    return st;
  };
  double temp = 2.0;
  // 400 proposals per slot, capped at 1024 slots' worth: mechanisms of thousands of reactions would
  // otherwise spend seconds of host time per ckmi_mech_create (round-4 advice); the GRI-3.0 (384 slots)
  // and 161-species (512) images are annealed exactly as before
  const int iters = 400 * std::min(n, 1024);
  for (int it = 0; it < iters; ++it, temp = std::max(0.05, temp * (1.0 - 6.0 / iters))) {
    const int a = (int)(rnd() % n);
    if (slots[a] < 0) continue;
    int b = -1;
    Rx save_a = rx[slots[a]];
    if (rnd() & 1) {  // swap two lanes of one block
      b = (int)(rnd() % n);
      if (b == a || slots[b] < 0 || blk[slots[b]] != blk[slots[a]]) continue;
      std::swap(slots[a], slots[b]);
    } else {  // swap two unit slots of one side of one reaction
      Rx& r = rx[slots[a]];
      const int side = (int)(rnd() & 1);
      if (r.ns[side] < 2) continue;
      const int u = (int)(rnd() % r.ns[side]), v = (int)(rnd() % r.ns[side]);
      if (u == v || r.sp[side][u] == r.sp[side][v]) continue;
      std::swap(r.sp[side][u], r.sp[side][v]);
    }
    const int sa = a / WAVE, sb = b >= 0 ? b / WAVE : sa;
    const int ca = lanes::strip_cost(rx, slots, sa * WAVE), cb = sb != sa ? lanes::strip_cost(rx, slots, sb * WAVE) : 0;
    const int delta = ca + cb - cost[sa] - (sb != sa ? cost[sb] : 0);
    const double x = (double)(rnd() >> 11) * (1.0 / 9007199254740992.0);
    if (delta <= 0 || x < std::exp(-delta / temp)) {
      cost[sa] = ca;
      if (sb != sa) cost[sb] = cb;
    } else if (b >= 0) {
      std::swap(slots[a], slots[b]);
    } else {
      rx[slots[a]] = save_a;
    }
  }
  // the slot orders as permutations of the file's unit-slot expansion
  for (int i = 0; i < II; ++i) {
    Rx ref;
    for (int side = 0; side < 2; ++side) {
      const int ns = side == 0 ? d->nr[i] : d->np[i];
      const int32_t* sp = (side == 0 ? d->rsp : d->psp) + CKMI_SLOTS * i;
      const double* nu = (side == 0 ? d->rnu : d->pnu) + CKMI_SLOTS * i;
      int c = 0;
      for (int u = 0; u < ns && !rxn_general(d, i); ++u)
        for (int k = 0; k < (int)nu[u] && c < 4; ++k) ref.sp[side][c++] = (uint8_t)sp[u];
      bool used[4] = {false, false, false, false};
      for (int u = 0; u < rx[i].ns[side]; ++u)
        for (int v = 0; v < rx[i].ns[side]; ++v)
          if (!used[v] && ref.sp[side][v] == rx[i].sp[side][u]) {
            used[v] = true;
            perm[i][4 * side + u] = (uint8_t)v;
            break;
          }
    }
  }
}

// Pack the compact mechanism image (ckmi_image.hpp) from the device-slot tables.
int build_image(ckmi_mech* m, const ckmi_mech_desc* d, const std::vector<int>& slots, const std::vector<int>& flags,
                const std::vector<int>& nrp, const std::vector<int4>& rsp, const std::vector<int4>& psp,
                const std::vector<double>& rnu, const std::vector<double>& pnu, const std::vector<double>& lnA,
                const std::vector<double>& beta, const std::vector<double>& Ea, const std::vector<double>& lnA0,
                const std::vector<double>& beta0, const std::vector<double>& Ea0, const std::vector<double>& fp,
                const std::vector<double>& rlnA, const std::vector<double>& rbeta, const std::vector<double>& rEa,
                const std::vector<int>& tb, const std::vector<int>& gptr, const std::vector<int>& gsp,
                const std::vector<double>& geff, const std::vector<double>& wt, const std::vector<double>& rwt,
                const std::vector<std::array<uint8_t, 8>>& perm) {
  const int KK = m->KK, IIp = m->IIpad, G = m->G;
  const int KKp = (KK + 1 + WAVE - 1) / WAVE * WAVE;  // room for the dummy species slot
  const int sp_one = KKp - 1;                          // = SP_ONE (63) whenever KK <= 63
  if (KK > KK_IMAGE_MAX)
    return set_error(CKMI_ERR_UNSUPPORTED, "more than 255 species not supported by the mechanism image");
  std::vector<uint32_t> urs(IIp, 0), ups(IIp, 0), unu(IIp, 0), uinfo(IIp, 0);
  std::vector<double> aux;
  int naux = 0;
  for (int s = 0; s < IIp; ++s) {
    const int nr = nrp[s] & 0xff, np = nrp[s] >> 8;
    uint32_t a = 0, b = 0, nu = 0;
    const int* r4 = &rsp[s].x;
    const int* p4 = &psp[s].x;
    const bool gen = (flags[s] & RX_GEN) != 0;  // real coefficients: no unit slots, aux stream
    // unit-coefficient slots: a species with coefficient c occupies c slots
    int ns_r = 0, ns_p = 0;
    int ur[4] = {0, 0, 0, 0}, up[4] = {0, 0, 0, 0};  // unit slots in file order, then in assign_lanes' order
    for (int u = 0; u < nr && !gen; ++u) {
      const int c = (int)rnu[u * IIp + s];
      nu |= (uint32_t)std::min(c, 15) << (4 * u);
      for (int k = 0; k < c; ++k, ++ns_r)
        if (ns_r < 4) ur[ns_r] = r4[u];
    }
    for (int u = 0; u < np && !gen; ++u) {
      const int c = (int)pnu[u * IIp + s];
      nu |= (uint32_t)std::min(c, 15) << (16 + 4 * u);
      for (int k = 0; k < c; ++k, ++ns_p)
        if (ns_p < 4) up[ns_p] = p4[u];
    }
    if (ns_r > 4 || ns_p > 4)
      return set_error(CKMI_ERR_UNSUPPORTED, "more than 4 molecules (sum of coefficients) on a reaction side");
    const uint8_t* pm = slots[s] >= 0 ? perm[slots[s]].data() : nullptr;
    for (int u = 0; u < ns_r; ++u) a |= (uint32_t)ur[pm ? pm[u] : u] << (8 * u);
    for (int u = 0; u < ns_p; ++u) b |= (uint32_t)up[pm ? pm[4 + u] : u] << (8 * u);
    for (int u = ns_r; u < 4; ++u) a |= (uint32_t)sp_one << (8 * u);
    for (int u = ns_p; u < 4; ++u) b |= (uint32_t)sp_one << (8 * u);
    urs[s] = a;
    ups[s] = b;
    unu[s] = nu;
    const int fl = flags[s];
    const int type = fl & 3;
    uint32_t inf = (uint32_t)(fl & 0x7f) | ((uint32_t)ns_r << 7) | ((uint32_t)ns_p << 10) | (uint32_t)(fl & 0x2000) |
                   (uint32_t)(fl & RX_GEN) | (uint32_t)(fl & RX_ALT);
    if (slots[s] >= 0 && type == CKMI_RXN_PLOG && (fl & RX_ALT)) {
      // Chebyshev stream: NT, NP, 1/Tmin, 1/Tmax, log10 Pmin, log10 Pmax [dyn/cm2], then a[t][p]
      const int i = slots[s];
      const double* r = d->plog_par + 4 * d->plog_ptr[i];
      const int nt = (int)r[0], npr = (int)r[1];
      std::vector<double> rec{(double)nt, (double)npr, 1.0 / r[4], 1.0 / r[5], std::log10(r[6] * 1.01325e6),
                              std::log10(r[7] * 1.01325e6)};
      rec.insert(rec.end(), r + 8, r + 8 + nt * npr);
      rec.resize((rec.size() + AUXW - 1) / AUXW * AUXW, 0.0);
      aux.insert(aux.end(), rec.begin(), rec.end());
      inf |= (uint32_t)naux << 16;
      naux += (int)rec.size() / AUXW;
    } else if (slots[s] >= 0 && type == CKMI_RXN_PLOG) {
      // PLOG stream: npts, then (ln P, ln A, b, E/R) per point, over ceil((1 + 4 npts) / AUXW) records
      const int i = slots[s], p0 = d->plog_ptr[i], n = d->plog_ptr[i + 1] - p0;
      std::vector<double> rec{(double)n};
      rec.insert(rec.end(), d->plog_par + 4 * p0, d->plog_par + 4 * (p0 + n));
      rec.resize((rec.size() + AUXW - 1) / AUXW * AUXW, 0.0);
      aux.insert(aux.end(), rec.begin(), rec.end());
      inf |= (uint32_t)naux << 16;
      naux += (int)rec.size() / AUXW;
    } else if (slots[s] >= 0 && (type == 2 || (fl & 8) || gen || (fl & RX_ALT))) {
      // (a Landau-Teller reaction's record: low = B, C of LT; fp[0], fp[1] = B, C of RLT)
      double rec[AUXW] = {lnA0[s], beta0[s], Ea0[s], fp[0 * IIp + s], fp[1 * IIp + s], fp[2 * IIp + s],
                          fp[3 * IIp + s], fp[4 * IIp + s], rlnA[s], rbeta[s], rEa[s], 0.0};
      const int ft = (fl >> 4) & 7;
      if (ft == CKMI_FALL_TROE3 || ft == CKMI_FALL_TROE4) {  // exp(-T / T***), exp(-T / T*): store 1/T
        rec[4] = 1.0 / rec[4];
        rec[5] = 1.0 / rec[5];
      } else if (ft == CKMI_FALL_SRI) {  // exp(-T / c)
        rec[5] = 1.0 / rec[5];
      }
      aux.insert(aux.end(), rec, rec + AUXW);
      inf |= (uint32_t)naux << 16;
      ++naux;
      if (gen) {  // records naux..: nr, np, (species, nu, order) x 4 reactant and x 4 product slots
        const int i = slots[s];
        double grec[GEN_RECORDS * AUXW] = {(double)nr, (double)np};
        for (int u = 0; u < nr; ++u) {
          grec[2 + 3 * u] = d->rsp[CKMI_SLOTS * i + u];
          grec[3 + 3 * u] = d->rnu[CKMI_SLOTS * i + u];
          grec[4 + 3 * u] = d->ford ? d->ford[CKMI_SLOTS * i + u] : d->rnu[CKMI_SLOTS * i + u];
        }
        for (int u = 0; u < np; ++u) {
          grec[GEN_P + 3 * u] = d->psp[CKMI_SLOTS * i + u];
          grec[GEN_P + 1 + 3 * u] = d->pnu[CKMI_SLOTS * i + u];
          grec[GEN_P + 2 + 3 * u] = d->rord ? d->rord[CKMI_SLOTS * i + u] : d->pnu[CKMI_SLOTS * i + u];
        }
        aux.insert(aux.end(), grec, grec + GEN_RECORDS * AUXW);
        naux += GEN_RECORDS;
      }
    }
    uinfo[s] = inf;
  }
  if (naux == 0) aux.assign(AUXW, 0.0), naux = 1;
  std::vector<double> th(15 * KKp, 0.0), wtp(KKp, 0.0), rwtp(KKp, 0.0);
  for (int k = 0; k < KK; ++k) {
    th[0 * KKp + k] = d->thermo[17 * k + 1];
    for (int c = 0; c < 7; ++c) {
      th[(1 + c) * KKp + k] = d->thermo[17 * k + 3 + c];
      th[(8 + c) * KKp + k] = d->thermo[17 * k + 10 + c];
    }
    wtp[k] = wt[k];
    rwtp[k] = rwt[k];
  }
  std::vector<char> blob;
  auto put = [&](const void* p, size_t bytes) -> int {
    const int off = (int)blob.size();
    blob.insert(blob.end(), (const char*)p, (const char*)p + bytes);
    blob.resize(align16((int)blob.size()), 0);
    return off;
  };
  MechImage& I = m->img;
  I.KK = KK;
  I.KKp = KKp;
  I.sp_one = sp_one;
  I.II = m->II;
  I.IIp = IIp;
  I.G = G;
  I.naux = naux;
  I.o_th = put(th.data(), th.size() * 8);
  I.o_wt = put(wtp.data(), KKp * 8);
  I.o_rwt = put(rwtp.data(), KKp * 8);
  I.o_lnA = put(lnA.data(), IIp * 8);
  I.o_beta = put(beta.data(), IIp * 8);
  I.o_Ea = put(Ea.data(), IIp * 8);
  I.o_rsp = put(urs.data(), IIp * 4);
  I.o_psp = put(ups.data(), IIp * 4);
  I.o_nu = put(unu.data(), IIp * 4);
  I.o_info = put(uinfo.data(), IIp * 4);
  I.o_tb = put(tb.data(), IIp * 4);
  I.o_aux = put(aux.data(), aux.size() * 8);
  I.o_gptr = put(gptr.data(), gptr.size() * 4);
  const int zero = 0;
  const double dzero = 0.0;
  I.o_gsp = gsp.empty() ? put(&zero, 4) : put(gsp.data(), gsp.size() * 4);
  I.o_geff = geff.empty() ? put(&dzero, 8) : put(geff.data(), geff.size() * 8);
  // transposed dense efficiency table geffT[k][17] (64 species rows, stride 17: conflict-free) for
  // the wave kernel (a per-lane walk of the sparse lists measured 0.6 % slower); only for KK <= 63 and
  // G <= 16, and only while the 64-wide launch (12 waves) still fits the 160 KB of LDS with it, else a stub
  const size_t lds_with = blob.size() + 64 * 17 * 8 + 8 * E2T_N + 8 * (size_t)KKp + jscratch_bytes<64>() +
                          12 * (size_t)slice_bytes(G);
  const bool dense = KK <= SP_ONE && G <= 16 && lds_with <= 160 * 1024;
  std::vector<double> geffd(dense ? (size_t)64 * 17 : (size_t)2, 0.0);
  for (int g = 0; dense && g < G; ++g)
    for (int e = gptr[g]; e < gptr[g + 1]; ++e) geffd[(size_t)gsp[e] * 17 + g] = geff[e];
  I.o_geffd = put(geffd.data(), geffd.size() * 8);  // MechView::mgt() tells the two sizes apart
  {
    double e2t[E2T_N];  // 2^(j / E2T_N): E2T_N doubles fill the 64 LDS banks once (conflict-free gathers)
    for (int j = 0; j < E2T_N; ++j) e2t[j] = (double)std::exp2((long double)j / (long double)E2T_N);
    I.o_e2t = put(e2t, sizeof(e2t));
  }
  {
    // element counts of each species for the corrector's element projection, right after e2t (the kernels
    // address it as o_e2t + 8 E2T_N: no extra view field): u64 per species, byte e = the count of the
    // e-th element that occurs in the mechanism (m->npe of them, <= CKMI_PROJ_MMAX; none otherwise)
    std::vector<uint64_t> el(KKp, 0ull);
    m->npe = 0;
    if (d->ncf && d->MM > 0) {
      std::vector<int> used;
      for (int e = 0; e < d->MM; ++e)
        for (int k = 0; k < KK; ++k)
          if (d->ncf[(size_t)e * KK + k] > 0) {
            used.push_back(e);
            break;
          }
      if ((int)used.size() <= CKMI_PROJ_MMAX) {
        m->npe = (int)used.size();
        for (int j = 0; j < m->npe; ++j)
          for (int k = 0; k < KK; ++k)
            el[k] |= (uint64_t)std::min(255, std::max(0, (int)d->ncf[(size_t)used[j] * KK + k])) << (8 * j);
      }
    }
    const int o_el = put(el.data(), el.size() * 8);
    if (o_el != I.o_e2t + 8 * E2T_N) return set_error(CKMI_ERR_ARG, "image layout: element table not after e2t");
  }
  I.bytes = (int)blob.size();
  {
    const int* so = nullptr;
    if (upload(m, m->slot_of, &so) != CKMI_OK) return CKMI_ERR_HIP;
    I.slot_of = so;
  }
  {
    // Jacobian column lists of the workgroup kernel (ckmi_big.hip rhs_big): for species j the unit slots
    // naming j, in device-slot order, so that a column block visits only its own slots instead of every
    // slot of every reaction once per block
    std::vector<std::vector<uint32_t>> lists(KK);
    for (int i = 0; i < IIp; ++i) {
      const uint32_t inf = uinfo[i];
      if (inf & RX_GEN) continue;
      const int nr = (inf >> 7) & 7, np = (inf >> 10) & 7;
      for (int sl = 0; sl < 8; ++sl) {
        const bool prod = sl >= 4;
        const int u0 = sl & 3;
        if (u0 >= (prod ? np : nr)) continue;
        const int j = (int)(((prod ? ups[i] : urs[i]) >> (8 * u0)) & 0xffu);
        if (j < KK) lists[j].push_back((uint32_t)i | ((uint32_t)sl << 16));
      }
    }
    std::vector<int> ptr(KK + 1, 0);
    std::vector<uint32_t> ent;
    for (int j = 0; j < KK; ++j) {
      ent.insert(ent.end(), lists[j].begin(), lists[j].end());
      ptr[j + 1] = (int)ent.size();
    }
    if (ent.empty()) ent.push_back(0u);
    const int* dp = nullptr;
    const uint32_t* de = nullptr;
    if (upload(m, ptr, &dp) != CKMI_OK || upload(m, ent, &de) != CKMI_OK) return CKMI_ERR_HIP;
    I.jcol_ptr = dp;
    I.jcol_ent = de;
  }
  void* p = nullptr;
  CKMI_HIP_CHECK(hipMalloc(&p, blob.size()));
  m->allocs.push_back(p);
  CKMI_HIP_CHECK(hipMemcpy(p, blob.data(), blob.size(), hipMemcpyHostToDevice));
  I.blob = (const uint4*)p;
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
  hipLaunchKernelGGL((rop_kernel<MODE, NCH, PL>), dim3(grid), dim3(NW * WAVE), lds, stream, m->img, m->d.orig, n, T, P,
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
  const int KK = d->KK, II = d->II;
  if (KK <= 0 || II < 0) return set_error(CKMI_ERR_SIZE, "bad sizes");
  if (KK > KK_IMAGE_MAX) return set_error(CKMI_ERR_UNSUPPORTED, "more than 255 species not supported by this build");
  // slot counts and species indices first: everything below (rxn_general, the slot classes, the
  // image) reads [4 i + u] for u < nr[i] / np[i]
  if (const char* bad = ckmi::check_slots(d)) return set_error(CKMI_ERR_ARG, bad);
  auto* m = new ckmi_mech();
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) {
    delete m;
    return set_error(CKMI_ERR_HIP, "no HIP device");
  }
  m->device = dev;
  m->KK = KK;
  m->II = II;
  {  // runaway guard range from the NASA-7 fits
    double tlo = 1e300, thi = 0.0;
    for (int k = 0; k < KK; ++k) {
      tlo = std::min(tlo, d->thermo[17 * k + 0]);
      thi = std::max(thi, d->thermo[17 * k + 2]);
    }
    m->tguard_lo = 0.5 * tlo;
    m->tguard_hi = 2.0 * thi;  // margin: legitimately hot runs extrapolate the fits (runaways reach 8-10k K)
  }
  // ---- order reactions: elementary, then third-body, then falloff
  std::vector<int> ordr;
  // strips stay type-uniform: chemically activated reactions run in the falloff strips
  // within a type, reactions with at most 2 unit slots per side first: the strips that hold only
  // those skip the slot-2/3 gathers wave-uniformly (eval_rxn_img); general reactions last
  auto slot_class = [&](int i) -> int {
    if (rxn_general(d, i)) return 2;
    double ur = 0.0, up = 0.0;
    for (int u = 0; u < d->nr[i]; ++u) ur += d->rnu[CKMI_SLOTS * i + u];
    for (int u = 0; u < d->np[i]; ++u) up += d->pnu[CKMI_SLOTS * i + u];
    return (ur > 2.0 || up > 2.0) ? 1 : 0;
  };
  std::vector<int> blk(II, -1);  // (rtype, slot class) block of each reaction: lanes swap within one
  for (int t : {CKMI_RXN_ELEMENTARY, CKMI_RXN_LT, CKMI_RXN_THIRDBODY, CKMI_RXN_FALLOFF, CKMI_RXN_CHEMACT, CKMI_RXN_PLOG,
                CKMI_RXN_CHEB})
    for (int cls = 0; cls < 3; ++cls)
      for (int i = 0; i < II; ++i)
        if (d->rtype[i] == t && slot_class(i) == cls) {
          ordr.push_back(i);
          blk[i] = 8 * t + cls;
        }
  for (int i = 0; i < II; ++i) {
    if (d->rtype[i] < 0 || d->rtype[i] > CKMI_RXN_LT) {
      delete m;
      return set_error(CKMI_ERR_UNSUPPORTED, "unsupported reaction type");
    }
    if (d->rtype[i] == CKMI_RXN_CHEB) {
      const int p0 = d->plog_ptr ? d->plog_ptr[i] : 0, nrow = d->plog_ptr ? d->plog_ptr[i + 1] - p0 : 0;
      const double* r = d->plog_par ? d->plog_par + 4 * p0 : nullptr;
      const int nt = r && nrow >= 2 ? (int)r[0] : 0, npr = r && nrow >= 2 ? (int)r[1] : 0;
      const bool ok = r && nt >= 1 && nt <= 12 && npr >= 1 && npr <= 12 && nrow == 2 + (nt * npr + 3) / 4 &&
                      r[4] > 0.0 && r[5] > r[4] && r[6] > 0.0 && r[7] > r[6] && !d->has_rev[i];
      if (!ok) {
        delete m;
        return set_error(CKMI_ERR_UNSUPPORTED, "Chebyshev record must hold 1..12 x 1..12 coefficients, increasing "
                                          "positive ranges and no REV");
      }
    }
    if (d->rtype[i] == CKMI_RXN_PLOG) {
      const int p0 = d->plog_ptr ? d->plog_ptr[i] : 0, n = d->plog_ptr ? d->plog_ptr[i + 1] - p0 : 0;
      bool ok = d->plog_par && n >= 1 && n <= 64 && !d->has_rev[i];
      for (int j = 0; ok && j + 1 < n; ++j) ok = d->plog_par[4 * (p0 + j)] < d->plog_par[4 * (p0 + j + 1)];
      if (!ok) {
        delete m;
        return set_error(CKMI_ERR_UNSUPPORTED, "PLOG table must hold 1..64 points with ascending pressures and no REV");
      }
    }
  }
  // pad the elementary block to a 64 multiple when it does not add a strip
  int nelem = 0;
  for (int i = 0; i < II; ++i) nelem += d->rtype[i] == 0;
  std::vector<int> slots;  // device slot -> original index (-1 pad)
  const int strips_nopad = (II + WAVE - 1) / WAVE;
  const int elem_pad = (nelem + WAVE - 1) / WAVE * WAVE;
  const int strips_pad = (elem_pad + (II - nelem) + WAVE - 1) / WAVE;
  const bool pad = nelem > 0 && nelem < II && strips_pad == strips_nopad;
  for (int s = 0; s < (int)ordr.size(); ++s) {
    if (pad && s == nelem)
      while ((int)slots.size() < elem_pad) slots.push_back(-1);
    slots.push_back(ordr[s]);
  }
  const int IIpad = std::max(WAVE, (int)((slots.size() + WAVE - 1) / WAVE * WAVE));
  while ((int)slots.size() < IIpad) slots.push_back(-1);
  std::vector<std::array<uint8_t, 8>> perm;
  {
    const char* e = std::getenv("CKMI_LANES");  // A/B knob: CKMI_LANES=0 keeps the file order
    if (e && e[0] == '0') perm.assign(II, {0, 1, 2, 3, 0, 1, 2, 3});
    else assign_lanes(d, slots, blk, perm);
  }
  m->IIpad = IIpad;
  m->slot_of.assign(II, -1);
  // ---- third-body groups (distinct efficiency lists)
  std::map<std::vector<std::pair<int, double>>, int> gmap;
  std::vector<int> gptr{0}, gsp;
  std::vector<double> geff;
  auto group_of = [&](int i) -> int {
    std::vector<std::pair<int, double>> key;
    for (int p = d->eff_ptr[i]; p < d->eff_ptr[i + 1]; ++p)
      if (d->eff_val[p] != 1.0) key.push_back({d->eff_sp[p], d->eff_val[p] - 1.0});
    std::sort(key.begin(), key.end());
    auto it = gmap.find(key);
    if (it != gmap.end()) return it->second;
    const int gid = (int)gmap.size();
    gmap[key] = gid;
    for (auto& kv : key) {
      gsp.push_back(kv.first);
      geff.push_back(kv.second);
    }
    gptr.push_back((int)gsp.size());
    return gid;
  };
  std::vector<int> flags(IIpad, 0), nrp(IIpad, 0), tb(IIpad, -1), orig(IIpad, -1);
  std::vector<int4> rsp(IIpad), psp(IIpad);
  std::vector<double> rnu(SLOTS * IIpad, 0.0), pnu(SLOTS * IIpad, 0.0);
  std::vector<double> lnA(IIpad, 0.0), beta(IIpad, 0.0), Ea(IIpad, 0.0), lnA0(IIpad, 0.0), beta0(IIpad, 0.0),
      Ea0(IIpad, 0.0), fp(5 * IIpad, 1.0), rlnA(IIpad, 0.0), rbeta(IIpad, 0.0), rEa(IIpad, 0.0), dnu(IIpad, 0.0),
      ordf(IIpad, 0.0), ordrr(IIpad, 0.0);
  for (int s = 0; s < IIpad; ++s) {
    rsp[s] = make_int4(0, 0, 0, 0);
    psp[s] = make_int4(0, 0, 0, 0);
    const int i = slots[s];
    orig[s] = i;
    if (i < 0) continue;
    m->slot_of[i] = s;
    const bool chemact = d->rtype[i] == CKMI_RXN_CHEMACT;  // device type 2 + info bit 13
    const bool cheb = d->rtype[i] == CKMI_RXN_CHEB;        // device type 3 (rate from the aux stream) + bit 15
    const bool lt = d->rtype[i] == CKMI_RXN_LT;            // device type 0 + bit 15 (B, C in the aux record)
    const int type = chemact ? CKMI_RXN_FALLOFF : (cheb ? CKMI_RXN_PLOG : (lt ? CKMI_RXN_ELEMENTARY : d->rtype[i]));
    flags[s] = type | (d->rev[i] ? 4 : 0) | (d->has_rev[i] ? 8 : 0) | ((d->ftype[i] & 7) << 4) | (chemact ? 0x2000 : 0) |
               ((cheb || lt) ? (int)RX_ALT : 0);
    const int nr = d->nr[i], np = d->np[i];
    if (rxn_general(d, i)) {  // FORD / RORD / non-integral: real coefficients, extended variants
      if (type == CKMI_RXN_PLOG || lt) {
        delete m;
        return set_error(CKMI_ERR_UNSUPPORTED,
                    "FORD / RORD or non-integral coefficients on a PLOG, Chebyshev or Landau-Teller reaction");
      }
      for (int u = 0; u < nr; ++u)
        if (!(d->rnu[i * CKMI_SLOTS + u] > 0.0) || (d->ford && d->ford[i * CKMI_SLOTS + u] < 0.0)) {
          delete m;
          return set_error(CKMI_ERR_UNSUPPORTED, "stoichiometric coefficients must be > 0 and orders >= 0");
        }
      for (int u = 0; u < np; ++u)
        if (!(d->pnu[i * CKMI_SLOTS + u] > 0.0) || (d->rord && d->rord[i * CKMI_SLOTS + u] < 0.0)) {
          delete m;
          return set_error(CKMI_ERR_UNSUPPORTED, "stoichiometric coefficients must be > 0 and orders >= 0");
        }
      flags[s] |= RX_GEN;
    }
    if (nr > GEN_SLOTS || np > GEN_SLOTS || ((nr > SLOTS || np > SLOTS) && !(flags[s] & RX_GEN))) {
      delete m;
      return set_error(CKMI_ERR_UNSUPPORTED, "more than 8 species on a reaction side");
    }
    nrp[s] = nr | (np << 8);
    int rr[4] = {0, 0, 0, 0}, pp[4] = {0, 0, 0, 0};
    double sf = 0.0, sr = 0.0;
    // per-slot device arrays hold the first SLOTS species (a general reaction reads its aux stream)
    for (int u = 0; u < nr; ++u) {
      if (u < SLOTS) {
        rr[u] = d->rsp[i * CKMI_SLOTS + u];
        rnu[u * IIpad + s] = d->rnu[i * CKMI_SLOTS + u];
      }
      sf += d->rnu[i * CKMI_SLOTS + u];
    }
    for (int u = 0; u < np; ++u) {
      if (u < SLOTS) {
        pp[u] = d->psp[i * CKMI_SLOTS + u];
        pnu[u * IIpad + s] = d->pnu[i * CKMI_SLOTS + u];
      }
      sr += d->pnu[i * CKMI_SLOTS + u];
    }
    rsp[s] = make_int4(rr[0], rr[1], rr[2], rr[3]);
    psp[s] = make_int4(pp[0], pp[1], pp[2], pp[3]);
    dnu[s] = sr - sf;
    ordf[s] = sf;
    ordrr[s] = sr;
    const bool plog = type == CKMI_RXN_PLOG;  // PLOG / CHEB: rate from the aux stream; the slot holds ln 1, 0, 0
    lnA[s] = plog ? 0.0 : d->arr[3 * i];
    beta[s] = plog ? 0.0 : d->arr[3 * i + 1];
    Ea[s] = plog ? 0.0 : d->arr[3 * i + 2];
    lnA0[s] = d->low[3 * i];
    beta0[s] = d->low[3 * i + 1];
    Ea0[s] = d->low[3 * i + 2];
    for (int c = 0; c < 5; ++c) fp[c * IIpad + s] = d->fpar[5 * i + c];
    rlnA[s] = d->revp[3 * i];
    rbeta[s] = d->revp[3 * i + 1];
    rEa[s] = d->revp[3 * i + 2];
    if (type == 1 || type == 2) tb[s] = d->tbsp[i] >= 0 ? -(d->tbsp[i] + 2) : group_of(i);
  }
  m->G = (int)gmap.size();
  m->rtype_orig.assign(d->rtype, d->rtype + II);
  // PLOG and chemically activated reactions are evaluated by the extended kernel variant
  m->has_plog = std::count(d->rtype, d->rtype + II, (int32_t)CKMI_RXN_PLOG) > 0 ||
                std::count(d->rtype, d->rtype + II, (int32_t)CKMI_RXN_CHEMACT) > 0 ||
                std::count(d->rtype, d->rtype + II, (int32_t)CKMI_RXN_CHEB) > 0 ||
                std::count(d->rtype, d->rtype + II, (int32_t)CKMI_RXN_LT) > 0;
  for (int i = 0; i < II; ++i) m->has_general = m->has_general || rxn_general(d, i);
  m->has_plog = m->has_plog || m->has_general;
  m->lnA_orig.resize(II);
  m->b_orig.resize(II);
  m->E_orig.resize(II);
  for (int i = 0; i < II; ++i) {
    m->lnA_orig[i] = d->arr[3 * i];
    m->b_orig[i] = d->arr[3 * i + 1];
    m->E_orig[i] = d->arr[3 * i + 2];
  }
  std::vector<double> wt(d->wt, d->wt + KK), rwt(KK), th(17 * KK);
  for (int k = 0; k < KK; ++k) {
    rwt[k] = 1.0 / wt[k];
    for (int c = 0; c < 17; ++c) th[c * KK + k] = d->thermo[17 * k + c];
  }
  MechDev& D = m->d;
  D.KK = KK;
  D.II = II;
  D.IIpad = IIpad;
  D.G = m->G;
  int rc = 0;
  rc |= upload(m, wt, &D.wt);
  rc |= upload(m, rwt, &D.rwt);
  rc |= upload(m, th, &D.th);
  rc |= upload(m, flags, &D.flags);
  rc |= upload(m, nrp, &D.nrp);
  rc |= upload(m, rsp, &D.rsp);
  rc |= upload(m, psp, &D.psp);
  rc |= upload(m, rnu, &D.rnu);
  rc |= upload(m, pnu, &D.pnu);
  rc |= upload(m, lnA, &D.lnA);
  rc |= upload(m, beta, &D.beta);
  rc |= upload(m, Ea, &D.Ea);
  rc |= upload(m, lnA0, &D.lnA0);
  rc |= upload(m, beta0, &D.beta0);
  rc |= upload(m, Ea0, &D.Ea0);
  rc |= upload(m, fp, &D.fp);
  rc |= upload(m, rlnA, &D.rlnA);
  rc |= upload(m, rbeta, &D.rbeta);
  rc |= upload(m, rEa, &D.rEa);
  rc |= upload(m, dnu, &D.dnu);
  rc |= upload(m, ordf, &D.ordf);
  rc |= upload(m, ordrr, &D.ordr);
  rc |= upload(m, tb, &D.tb);
  rc |= upload(m, orig, &D.orig);
  rc |= upload(m, gptr, &D.gptr);
  rc |= upload(m, gsp, &D.gsp);
  rc |= upload(m, geff, &D.geff);
  rc |= build_image(m, d, slots, flags, nrp, rsp, psp, rnu, pnu, lnA, beta, Ea, lnA0, beta0, Ea0, fp, rlnA, rbeta, rEa,
                    tb, gptr, gsp, geff, wt, rwt, perm);
  if (rc) {
    ckmi_mech_destroy(m);
    return rc;
  }
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
      if (upload(m, prm, &p)) {
        ckmi_mech_destroy(m);
        return CKMI_ERR_HIP;
      }
      m->jit->prm = const_cast<double*>(p);
      if (const char* dump = std::getenv("CKMI_JIT_DUMP")) {
        if (FILE* f = std::fopen(dump, "w")) {
          std::fputs(m->jit->src.c_str(), f);
          std::fclose(f);
        }
      }
    }
  }
  *out = m;
  return CKMI_OK;
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
  CKMI_HIP_CHECK(hipMemcpy(const_cast<double*>(m->d.lnA) + s, &lnA, sizeof(double), hipMemcpyHostToDevice));
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
