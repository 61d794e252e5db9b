// ckmi_network.hip -- batched networks of steady-state PSRs with recycle streams (ckmi_psr_network_run,
// include/ckmi.h).  The coupling only: the flow balance, the stream mixing in front of every
// reactor position, the scatter of a position's solutions, the tear test and the stable compaction of the
// active list.  The reactors themselves are solved by ckmi_psr_run, one launch per position and sweep.
#include <algorithm>
#include <cmath>
#include <string>

#include "ckmi_internal.hpp"

using namespace ckmi;

namespace {
constexpr int RMAX = CKMI_NET_RMAX;
constexpr int NET_BLOCK = 256;  // 4 waves: one wave per network in the mixing, scatter and tear kernels
constexpr int NET_WAVES = NET_BLOCK / WAVE;
constexpr int NO_INLET = -1;  // member status of a reactor no stream reaches in the first sweep

// every array of one call; the c* arrays are the compacted launch arrays, indexed by the slot in the active list
struct NetIO {
  int n_net, R, E, KK;
  const double *P, *split, *ext_mdot, *ext_T, *ext_Y, *tau_or_vol, *Tguess, *Yguess;
  const int* tear;
  double *Tss, *Yss, *mdot, *rho, *tau_res, *vol, *resid;
  int *stats, *net_stats;
  double* tear_resid;
  int *live, *act, *count;  // live[n_net]: still iterating; act[n_net]: the active list; count: its length
  double *Tprev, *Yprev;    // [n_net][R], [n_net][R][KK]: the last sweep's solutions
  double *cP, *cTin, *cYin, *cmdot, *ctv, *cTg, *cYg, *cTss, *cYss, *crho, *ctau, *cvol, *cresid;
  int* cstats;
};

// (a) flow balance: one lane per network.  (I - F^T) mdot = mdot_ext by partially pivoted elimination; also the
// feed-forward flag, and NaN in every per-reactor output so that a position never reached reads as not solved
__global__ __launch_bounds__(NET_BLOCK) void net_flow_kernel(NetIO io) {
  const int net = blockIdx.x * NET_BLOCK + threadIdx.x;
  if (net >= io.n_net) return;
  const int R = io.R, E = io.E, KK = io.KK;
  const double* S = io.split + (size_t)net * R * (R + 1);
  double A[RMAX][RMAX + 1], colmax[RMAX];
  bool ff = true;
  int ntear = 0;
  for (int i = 0; i < R; ++i) {
    for (int j = 0; j < R; ++j) {
      const double f = S[j * (R + 1) + i];
      A[i][j] = (i == j ? 1.0 : 0.0) - f;
      if (j >= i && f != 0.0) ff = false;
    }
    double me = 0.0;
    for (int e = 0; e < E; ++e) me += io.ext_mdot[((size_t)net * R + i) * E + e];
    A[i][R] = me;
    ntear += io.tear[(size_t)net * R + i] != 0;
  }
  for (int c = 0; c < R; ++c) {
    double mx = 0.0;
    for (int i = 0; i < R; ++i) mx = fmax(mx, fabs(A[i][c]));
    colmax[c] = mx;
  }
  bool ok = true;
  for (int c = 0; c < R && ok; ++c) {
    int p = c;
    for (int r = c + 1; r < R; ++r)
      if (fabs(A[r][c]) > fabs(A[p][c])) p = r;
    const double piv = A[p][c];
    if (!(fabs(piv) > 0.0) || !(fabs(piv) >= 1e-12 * colmax[c])) {
      ok = false;
      break;
    }
    if (p != c)
      for (int j = c; j <= R; ++j) {
        const double t = A[c][j];
        A[c][j] = A[p][j];
        A[p][j] = t;
      }
    for (int r = c + 1; r < R; ++r) {
      const double l = A[r][c] / piv;
      if (l != 0.0)
        for (int j = c; j <= R; ++j) A[r][j] -= l * A[c][j];
    }
  }
  double md[RMAX];
  if (ok) {
    for (int i = R - 1; i >= 0; --i) {
      double s = A[i][R];
      for (int j = i + 1; j < R; ++j) s -= A[i][j] * md[j];
      md[i] = s / A[i][i];
      if (!(md[i] > 0.0) || !(md[i] < 1e300)) ok = false;  // a reactor nothing flows through
    }
  }
  const double nan = __builtin_nan("");
  for (int i = 0; i < R; ++i) {
    const size_t ri = (size_t)net * R + i;
    io.mdot[ri] = ok ? md[i] : nan;
    io.Tss[ri] = io.rho[ri] = io.tau_res[ri] = io.vol[ri] = io.resid[ri] = nan;
    for (int k = 0; k < KK; ++k) io.Yss[ri * KK + k] = nan;
    for (int q = 0; q < CKMI_NSTAT; ++q) io.stats[ri * CKMI_NSTAT + q] = 0;
  }
  int* ns = io.net_stats + (size_t)net * CKMI_NET_NSTAT;
  ns[CKMI_NET_STAT_STATUS] = ok ? CKMI_NET_OK : CKMI_NET_FLOW_SINGULAR;
  ns[CKMI_NET_STAT_SWEEPS] = 0;
  ns[CKMI_NET_STAT_FLAGS] = (ff ? 1 : 0) | ((!ff && ntear == 0) ? 2 : 0);
  ns[3] = 0;
  io.tear_resid[net] = 0.0;
  io.live[net] = ok ? 1 : 0;
}

// stable compaction of the live networks into the active list: one wave walks the flags 64 at a time and places
// each live network behind the live ones before it (ballot + prefix count, no atomics), so the slot order is the
// network order whatever the batch
__global__ __launch_bounds__(WAVE) void net_compact_kernel(NetIO io) {
  const int lane = threadIdx.x;
  int total = 0;
  for (int base = 0; base < io.n_net; base += WAVE) {
    const int i = base + lane;
    const bool f = i < io.n_net && io.live[i] != 0;
    const unsigned long long mask = __ballot(f);
    if (f) io.act[total + __popcll(mask & ((1ull << lane) - 1ull))] = i;
    total += __popcll(mask);
  }
  if (lane == 0) *io.count = total;
}

// (b) the effective inlet of position `pos`: one wave per active network, lanes over species.  Mass and enthalpy
// of the external slots and of the internal sources that have a solution (every reactor after the first sweep, the
// upstream ones in it); T_in by Newton on sum_k Y_in,k h_k(T) = H_in.  One source alone is passed through as it is.
// gmode / mode: the position's guess mode and PSR mode (the latter only shapes the placeholder of a stopped network)
__global__ __launch_bounds__(NET_BLOCK) void net_mix_kernel(NetIO io, MechDev M, int n_act, int pos, int sweep,
                                                            int gmode, int mode) {
  const int s = blockIdx.x * NET_WAVES + threadIdx.x / WAVE;
  if (s >= n_act) return;
  const int lane = threadIdx.x % WAVE;
  const int R = io.R, E = io.E, KK = io.KK;
  const bool on = lane < KK;
  const int k = on ? lane : 0;
  const int net = io.act[s];
  const size_t ri = (size_t)net * R + pos;
  double ys = 0.0, hs = 0.0, msum = 0.0, tsum = 0.0, Tone = 0.0, yone = 0.0;
  int nsrc = 0;
  const bool alive = io.live[net] != 0;
  if (alive) {
    for (int e = 0; e < E; ++e) {
      const double m = io.ext_mdot[ri * E + e];
      if (m > 0.0) {
        const double T = io.ext_T[ri * E + e];
        const double y = on ? io.ext_Y[(ri * E + e) * KK + k] : 0.0;
        const double h = nasa7(M, k, T, 0.0).hRT * RU * T * M.rwt[k];
        ys += m * y, hs += m * y * h, msum += m, tsum += m * T, Tone = T, yone = y, ++nsrc;
      }
    }
    for (int j = 0; j < R; ++j) {
      if (sweep == 0 && j >= pos) continue;
      const size_t rj = (size_t)net * R + j;
      const double f = io.split[rj * (R + 1) + pos];
      if (f > 0.0) {
        const double m = f * io.mdot[rj];
        const double T = io.Tss[rj];
        const double y = on ? io.Yss[rj * KK + k] : 0.0;
        const double h = nasa7(M, k, T, 0.0).hRT * RU * T * M.rwt[k];
        ys += m * y, hs += m * y * h, msum += m, tsum += m * T, Tone = T, yone = y, ++nsrc;
      }
    }
  }
  if (nsrc == 0) {
    // a stopped network keeps its slot until the sweep ends: it gets a reactor that is steady at once (cold pure
    // species 0) and the scatter skips it.  A live network without any inlet stream stops here.
    if (alive && lane == 0) {
      io.live[net] = 0;
      io.net_stats[(size_t)net * CKMI_NET_NSTAT + CKMI_NET_STAT_STATUS] = CKMI_NET_REACTOR_FAILED;
      io.net_stats[(size_t)net * CKMI_NET_NSTAT + CKMI_NET_STAT_SWEEPS] = sweep + 1;
      io.stats[ri * CKMI_NSTAT + CKMI_STAT_STATUS] = NO_INLET;
    }
    const double y = lane == 0 ? 1.0 : 0.0;
    if (on) io.cYin[(size_t)s * KK + k] = y, io.cYg[(size_t)s * KK + k] = y;
    if (lane == 0) {
      io.cP[s] = io.P[ri];
      io.cTin[s] = io.cTg[s] = 300.0;
      io.cmdot[s] = 1.0;
      io.ctv[s] = mode == 1 ? 1e-3 : 1.0;
    }
    return;
  }
  double Tin = Tone, yin = yone;
  if (nsrc > 1) {
    yin = ys / msum;
    const double H = wave_sum(on ? hs : 0.0) / msum;
    Tin = tsum / msum;
    for (int it = 0; it < 50; ++it) {
      const SpThermo t = nasa7(M, k, Tin, 0.0);
      const double h = wave_sum(on ? yin * t.hRT * RU * Tin * M.rwt[k] : 0.0);
      const double cp = wave_sum(on ? yin * t.cpR * RU * M.rwt[k] : 0.0);
      const double dT = (H - h) / cp;
      Tin += dT;
      if (fabs(dT) <= 1e-12 * Tin) break;
    }
  }
  if (on) {
    io.cYin[(size_t)s * KK + k] = yin;
    io.cYg[(size_t)s * KK + k] = sweep > 0 ? io.Yss[ri * KK + k] : (gmode == 1 ? yin : io.Yguess[ri * KK + k]);
  }
  if (lane == 0) {
    io.cP[s] = io.P[ri];
    io.cTin[s] = Tin;
    io.cmdot[s] = io.mdot[ri];
    io.ctv[s] = io.tau_or_vol[ri];
    io.cTg[s] = sweep > 0 ? io.Tss[ri] : io.Tguess[ri];
  }
}

// (d) the solutions of position `pos` back to [net][pos]; a reactor that did not reach a steady state stops its network
__global__ __launch_bounds__(NET_BLOCK) void net_scatter_kernel(NetIO io, int n_act, int pos, int sweep) {
  const int s = blockIdx.x * NET_WAVES + threadIdx.x / WAVE;
  if (s >= n_act) return;
  const int lane = threadIdx.x % WAVE;
  const int R = io.R, KK = io.KK;
  const int net = io.act[s];
  if (io.live[net] == 0) return;
  const size_t ri = (size_t)net * R + pos;
  if (lane < KK) io.Yss[ri * KK + lane] = io.cYss[(size_t)s * KK + lane];
  if (lane < CKMI_NSTAT) io.stats[ri * CKMI_NSTAT + lane] = io.cstats[(size_t)s * CKMI_NSTAT + lane];
  if (lane == 0) {
    io.Tss[ri] = io.cTss[s];
    io.rho[ri] = io.crho[s];
    io.tau_res[ri] = io.ctau[s];
    io.vol[ri] = io.cvol[s];
    io.resid[ri] = io.cresid[s];
    if (io.cstats[(size_t)s * CKMI_NSTAT + CKMI_STAT_STATUS] != CKMI_RUN_OK) {
      io.live[net] = 0;
      io.net_stats[(size_t)net * CKMI_NET_NSTAT + CKMI_NET_STAT_STATUS] = CKMI_NET_REACTOR_FAILED;
      io.net_stats[(size_t)net * CKMI_NET_NSTAT + CKMI_NET_STAT_SWEEPS] = sweep + 1;
    }
  }
}

// (e) end of a sweep: one wave per active network, lanes over species, a loop over the reactors.  The scaled change
// of every tear point since the last sweep, the relaxation, and who leaves the active list
__global__ __launch_bounds__(NET_BLOCK) void net_tear_kernel(NetIO io, int n_act, int sweep, int max_sweeps, double rtol,
                                                             double atol, double relax) {
  const int s = blockIdx.x * NET_WAVES + threadIdx.x / WAVE;
  if (s >= n_act) return;
  const int lane = threadIdx.x % WAVE;
  const int R = io.R, KK = io.KK;
  const bool on = lane < KK;
  const int net = io.act[s];
  if (io.live[net] == 0) return;
  int* ns = io.net_stats + (size_t)net * CKMI_NET_NSTAT;
  const int flags = ns[CKMI_NET_STAT_FLAGS];
  if (flags & 1) {  // feed-forward: one sweep, no tear test
    if (lane == 0) {
      ns[CKMI_NET_STAT_STATUS] = CKMI_NET_OK;
      ns[CKMI_NET_STAT_SWEEPS] = 1;
      io.live[net] = 0;
    }
    return;
  }
  double worst = 0.0;
  for (int r = 0; r < R; ++r) {
    const size_t rr = (size_t)net * R + r;
    double T = io.Tss[rr];
    double y = on ? io.Yss[rr * KK + lane] : 0.0;
    if (sweep > 0) {
      const double pT = io.Tprev[rr];
      const double py = on ? io.Yprev[rr * KK + lane] : 0.0;
      if (io.tear[rr] != 0 || (flags & 2)) {
        const double eT = fabs(T - pT) / (rtol * fabs(T));
        const double ey = fabs(y - py) / (atol + rtol * fabs(y));
        worst = fmax(worst, (eT == eT && ey == ey) ? fmax(eT, ey) : 1e300);
      }
      if (relax != 1.0) {
        T = pT + relax * (T - pT);
        y = py + relax * (y - py);
        if (on) io.Yss[rr * KK + lane] = y;
        if (lane == 0) io.Tss[rr] = T;
      }
    }
    if (on) io.Yprev[rr * KK + lane] = y;
    if (lane == 0) io.Tprev[rr] = T;
  }
  worst = wave_max(worst);
  if (lane == 0) {
    io.tear_resid[net] = worst;
    ns[CKMI_NET_STAT_SWEEPS] = sweep + 1;
    if (sweep > 0 && worst <= 1.0) {
      ns[CKMI_NET_STAT_STATUS] = CKMI_NET_OK;
      io.live[net] = 0;
    } else if (sweep + 1 >= max_sweeps) {
      ns[CKMI_NET_STAT_STATUS] = CKMI_NET_TEAR_LIMIT;
      io.live[net] = 0;
    }
  }
}

// the call's stream-ordered workspace and its pinned count, released on every way out
struct NetScratch {
  hipStream_t st;
  StreamWorkspace ws;
  int* hcount = nullptr;
  explicit NetScratch(hipStream_t stream) : st(stream), ws(stream) {}
  ~NetScratch() {
    if (hcount) (void)hipHostFree(hcount);
  }
};

int read_count(const NetIO& io, NetScratch& sc, int* n_act) {
  hipLaunchKernelGGL(net_compact_kernel, dim3(1), dim3(WAVE), 0, sc.st, io);
  CKMI_HIP_CHECK(hipGetLastError());
  CKMI_HIP_CHECK(hipMemcpyAsync(sc.hcount, io.count, sizeof(int), hipMemcpyDeviceToHost, sc.st));
  CKMI_HIP_CHECK(hipStreamSynchronize(sc.st));
  *n_act = *sc.hcount;
  if (*n_act < 0 || *n_act > io.n_net) return set_error(CKMI_ERR_HIP, "internal: active network count out of range");
  return CKMI_OK;
}
}  // namespace

extern "C" {

int ckmi_psr_network_run(const ckmi_mech* m, int32_t n_net, int32_t R, int32_t E, const ckmi_reactor_cfg* cfg,
                         const ckmi_psr_cfg* psr, const ckmi_network_cfg* net, const int32_t* guess_mode,
                         const double* P, const double* split, const double* ext_mdot, const double* ext_T,
                         const double* ext_Y, const double* tau_or_vol, const double* Tguess, const double* Yguess,
                         const int32_t* tear, double* Tss, double* Yss, double* mdot, double* rho, double* tau_res,
                         double* vol, double* resid, int32_t* stats, int32_t* net_stats, double* tear_resid,
                         void* stream) {
  if (!m || !cfg || !psr || !net || !guess_mode || n_net < 0 || R < 1 || E < 1) return set_error(CKMI_ERR_ARG, "bad argument");
  if (R > RMAX)
    return set_error(CKMI_ERR_UNSUPPORTED, "a network has at most " + std::to_string(RMAX) + " reactors, not " + std::to_string(R));
  if (m->KK + 1 > WAVE)
    return set_error(CKMI_ERR_UNSUPPORTED, "PSR networks need KK + 1 <= 64 (the wave-per-reactor kernel); this mechanism has " +
                                          std::to_string(m->KK) + " species");
  const int max_sweeps = net->max_sweeps == 0 ? 200 : net->max_sweeps;
  const double rtol = net->tear_rtol == 0.0 ? 1e-6 : net->tear_rtol, atol = net->tear_atol == 0.0 ? 1e-8 : net->tear_atol;
  const double relax = net->relax == 0.0 ? 1.0 : net->relax;
  if (max_sweeps < 1 || !(rtol > 0.0) || !(atol >= 0.0) || !(relax > 0.0))
    return set_error(CKMI_ERR_ARG, "max_sweeps must be >= 1, tear_rtol > 0, tear_atol >= 0 and relax > 0");
  for (int i = 0; i < R; ++i) {
    if (guess_mode[i] != 0 && guess_mode[i] != 1) return set_error(CKMI_ERR_ARG, "guess_mode must be 0 or 1");
    // an empty launch checks the position's configuration before anything runs
    const int rc = ckmi_psr_run(m, &cfg[i], &psr[i], 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, stream);
    if (rc) return rc;
  }
  if (n_net > 0 && (!P || !split || !ext_mdot || !ext_T || !ext_Y || !tau_or_vol || !Tguess || !Yguess || !tear || !Tss ||
                    !Yss || !mdot || !rho || !tau_res || !vol || !resid || !stats || !net_stats || !tear_resid))
    return set_error(CKMI_ERR_ARG, "every input and output array is required");
  if (n_net == 0) return CKMI_OK;
  const int KK = m->KK;
  NetScratch sc((hipStream_t)stream);
  const size_t n = (size_t)n_net;
  const size_t nd = n * ((size_t)R * (KK + 1) + 10 + 3 * (size_t)KK);  // doubles
  const size_t ni = n * (2 + CKMI_NSTAT) + 1;                           // ints
  if (int rc = sc.ws.alloc(nd * sizeof(double) + ni * sizeof(int))) return rc;
  CKMI_HIP_CHECK(hipHostMalloc((void**)&sc.hcount, sizeof(int), hipHostMallocDefault));
  NetIO io{};
  io.n_net = n_net, io.R = R, io.E = E, io.KK = KK;
  io.P = P, io.split = split, io.ext_mdot = ext_mdot, io.ext_T = ext_T, io.ext_Y = ext_Y, io.tau_or_vol = tau_or_vol;
  io.Tguess = Tguess, io.Yguess = Yguess, io.tear = tear;
  io.Tss = Tss, io.Yss = Yss, io.mdot = mdot, io.rho = rho, io.tau_res = tau_res, io.vol = vol, io.resid = resid;
  io.stats = stats, io.net_stats = net_stats, io.tear_resid = tear_resid;
  double* d = sc.ws.take<double>(nd * sizeof(double) + ni * sizeof(int));  // one piece, laid out below
  auto take = [&](size_t cnt) {
    double* p = d;
    d += cnt;
    return p;
  };
  io.Tprev = take(n * R), io.Yprev = take(n * R * KK);
  io.cP = take(n), io.cTin = take(n), io.cmdot = take(n), io.ctv = take(n), io.cTg = take(n);
  io.cTss = take(n), io.crho = take(n), io.ctau = take(n), io.cvol = take(n), io.cresid = take(n);
  io.cYin = take(n * KK), io.cYg = take(n * KK), io.cYss = take(n * KK);
  int* q = (int*)d;
  io.live = q, io.act = q + n, io.cstats = q + 2 * n, io.count = q + (2 + CKMI_NSTAT) * n;

  hipLaunchKernelGGL(net_flow_kernel, dim3((n_net + NET_BLOCK - 1) / NET_BLOCK), dim3(NET_BLOCK), 0, sc.st, io);
  CKMI_HIP_CHECK(hipGetLastError());
  int n_act = 0;
  int rc = read_count(io, sc, &n_act);
  if (rc) return rc;
  for (int sweep = 0; sweep < max_sweeps && n_act > 0; ++sweep) {
    const dim3 grid((n_act + NET_WAVES - 1) / NET_WAVES);
    for (int pos = 0; pos < R; ++pos) {
      hipLaunchKernelGGL(net_mix_kernel, grid, dim3(NET_BLOCK), 0, sc.st, io, m->d, n_act, pos, sweep, (int)guess_mode[pos],
                         (int)psr[pos].mode);
      CKMI_HIP_CHECK(hipGetLastError());
      rc = ckmi_psr_run(m, &cfg[pos], &psr[pos], n_act, io.cP, io.cTin, io.cYin, io.cmdot, io.ctv, io.cTg, io.cYg, io.cTss,
                        io.cYss, io.crho, io.ctau, io.cvol, io.cresid, io.cstats, stream);
      if (rc) return rc;
      hipLaunchKernelGGL(net_scatter_kernel, grid, dim3(NET_BLOCK), 0, sc.st, io, n_act, pos, sweep);
      CKMI_HIP_CHECK(hipGetLastError());
    }
    hipLaunchKernelGGL(net_tear_kernel, grid, dim3(NET_BLOCK), 0, sc.st, io, n_act, sweep, max_sweeps, rtol, atol, relax);
    CKMI_HIP_CHECK(hipGetLastError());
    rc = read_count(io, sc, &n_act);
    if (rc) return rc;
  }
  return CKMI_OK;
}

}  // extern "C"
