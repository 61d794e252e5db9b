// ckmi_equil.hip -- batched gas-phase chemical equilibrium and Chapman-Jouguet states (ckmi_equil_run,
// include/ckmi.h).  Ideal gas, element potentials, one Newton system for the ten Chemkin
// options (the reduced Gordon-McBride iteration in ln n_j, ln n, ln T, ln P).
//
// Mapping: one state per lane, 256-lane blocks that walk the batch in tiles.  The species loop is
// wave-uniform; the per-species table (NASA-7 coefficients, molar mass, element counts) sits in LDS and is
// read as a broadcast.  The K values ln n_j of a lane live in a [species][lane] global work space (coalesced),
// never in a per-thread array, and each pass loads the next species' values before it stores this one's; the reduced (MM + 3)-row system is assembled and solved in registers with
// every index a compile-time constant (templated on the element count MM), partial pivoting by selects.
// A lane that has converged idles under the execution mask until its wave has.
#include <algorithm>
#include <cstring>
#include <mutex>

#include "ckmi_internal.hpp"

using namespace ckmi;

namespace {

constexpr int EQ_BLOCK = 256;
// table row of one species: tmid, low a1..a7, high a1..a7, W, element counts (u64, byte e), element mask
constexpr int EQ_ROW = 18;
constexpr int EQ_TMID = 0, EQ_LOW = 1, EQ_HIGH = 8, EQ_WT = 15, EQ_EL = 16, EQ_MASK = 17;
constexpr double EQ_T_START = 3800.0;
constexpr double EQ_LN_N_START = -3.4011973816621555;  // ln(1 / 30) mol/g
constexpr double EQ_LN_RU_PATM = -LN_PATM_RU;          // ln(RU / PATM)

struct EqArgs {
  int n, KK;
  const double* tab;  // [KK][EQ_ROW]
  const int32_t* option;
  const double *T, *P, *Y;
  double *Teq, *Peq, *Yeq, *sound, *det;
  int32_t* stats;
  double* ws;  // 3 x [KK][gridDim.x * EQ_BLOCK]: ln n_j, its pending correction, n_j
  double tol;
  int max_iter;
  double cj_vlo, cj_vhi, cj_start, cj_tol;
  int cj_iter;
};

// constraint kinds of the two option rows
enum { K_T = 0, K_P = 1, K_V = 2, K_H = 3, K_U = 4, K_S = 5, K_J = 6 };

__device__ __forceinline__ uint64_t bits_of(double v) { return (uint64_t)__double_as_longlong(v); }
__device__ __forceinline__ uint32_t uni_mask(double v) {
  return (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)bits_of(v));
}
__device__ __forceinline__ uint64_t uni_u64(double v) {
  const uint64_t b = bits_of(v);
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)b);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(b >> 32));
  return ((uint64_t)hi << 32) | lo;
}

// cp/R, h/RT, s/R of the species of `row` (LDS) at T
__device__ __forceinline__ void nasa7(const double* row, double T, double lnT, double rT, double& C, double& H,
                                      double& S) {
  const int o = (T > row[EQ_TMID]) ? EQ_HIGH : EQ_LOW;
  const double a1 = row[o], a2 = row[o + 1], a3 = row[o + 2], a4 = row[o + 3], a5 = row[o + 4], a6 = row[o + 5],
               a7 = row[o + 6];
  C = a1 + T * (a2 + T * (a3 + T * (a4 + T * a5)));
  H = a1 + T * (a2 * 0.5 + T * (a3 * (1.0 / 3.0) + T * (a4 * 0.25 + T * (a5 * 0.2)))) + a6 * rT;
  S = a1 * lnT + T * (a2 + T * (a3 * 0.5 + T * (a4 * (1.0 / 3.0) + T * (a5 * 0.25)))) + a7;
}

// In-register Gaussian elimination with partial pivoting of the N x N system with two right-hand sides
// (columns N and N + 1); every index is a compile-time constant after unrolling, the row exchange is a
// select.  Returns the solutions in x (first right-hand side) and the last entry of the second.
template <int N>
__device__ __forceinline__ void solve2(double (&M)[N][N + 2], double (&x)[N], double& x2_last) {
#pragma unroll
  for (int k = 0; k < N; ++k) {
    double best = fabs(M[k][k]);
    int pr = k;
#pragma unroll
    for (int r = k + 1; r < N; ++r) {
      const double v = fabs(M[r][k]);
      if (v > best) {
        best = v;
        pr = r;
      }
    }
#pragma unroll
    for (int r = k + 1; r < N; ++r) {
      const bool sw = pr == r;
#pragma unroll
      for (int c = k; c < N + 2; ++c) {
        const double t = M[k][c];
        M[k][c] = sw ? M[r][c] : t;
        M[r][c] = sw ? t : M[r][c];
      }
    }
    const double inv = 1.0 / M[k][k];
#pragma unroll
    for (int c = k + 1; c < N + 2; ++c) M[k][c] *= inv;
#pragma unroll
    for (int r = k + 1; r < N; ++r) {
      const double f = M[r][k];
#pragma unroll
      for (int c = k + 1; c < N + 2; ++c) M[r][c] = fma(-f, M[k][c], M[r][c]);
    }
  }
  double x2[N];
#pragma unroll
  for (int k = N - 1; k >= 0; --k) {
    double s = M[k][N], s2 = M[k][N + 1];
#pragma unroll
    for (int c = k + 1; c < N; ++c) {
      s = fma(-M[k][c], x[c], s);
      s2 = fma(-M[k][c], x2[c], s2);
    }
    x[k] = s;
    x2[k] = s2;
  }
  x2_last = x2[N - 1];
}

template <int MM>
__global__ __launch_bounds__(EQ_BLOCK) void equil_kernel(const EqArgs a) {
  extern __shared__ double tab[];  // [KK][EQ_ROW]
  constexpr int N = MM + 3, INU = MM, ITH = MM + 1, IP = MM + 2;
  const int KK = a.KK;
  for (int i = threadIdx.x; i < KK * EQ_ROW; i += EQ_BLOCK) tab[i] = a.tab[i];
  __syncthreads();
  const size_t stride = (size_t)gridDim.x * EQ_BLOCK;
  const size_t slot = (size_t)blockIdx.x * EQ_BLOCK + threadIdx.x;
  double* wy = a.ws + slot;                            // ln n_j
  // the pending correction of ln n_j: pass 2 writes it, the next pass 1 (or the output pass) applies it
  double* wd = a.ws + (size_t)KK * stride + slot;
  double* wn = a.ws + 2 * (size_t)KK * stride + slot;  // n_j

  const int ntiles = (a.n + EQ_BLOCK - 1) / EQ_BLOCK;
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int s = tile * EQ_BLOCK + (int)threadIdx.x;
    const bool valid = s < a.n;
    // ------------------------------------------------------------ the given state and what it holds
    const int opt = valid ? a.option[s] : 1;
    const double T0 = valid ? a.T[s] : 1000.0, P0 = valid ? a.P[s] : PATM;
    const double* __restrict__ Yg = a.Y + (size_t)(valid ? s : 0) * KK;
    int k1 = K_T, k2 = K_P;
    switch (opt) {
      case 1: k1 = K_T, k2 = K_P; break;
      case 2: k1 = K_T, k2 = K_V; break;
      case 3: k1 = K_T, k2 = K_S; break;
      case 4: k1 = K_P, k2 = K_V; break;
      case 5: k1 = K_P, k2 = K_H; break;
      case 6: k1 = K_P, k2 = K_S; break;
      case 7: k1 = K_V, k2 = K_U; break;
      case 8: k1 = K_V, k2 = K_H; break;
      case 9: k1 = K_V, k2 = K_S; break;
      case 10: k1 = K_V, k2 = K_J; break;
      default: break;
    }
    double b0[MM];
#pragma unroll
    for (int k = 0; k < MM; ++k) b0[k] = 0.0;
    double sumY = 0.0, n0 = 0.0;
    for (int j = 0; j < KK; ++j) {
      const double* row = tab + j * EQ_ROW;
      const double y = fmax(Yg[j], 0.0);
      const double nj = y / row[EQ_WT];
      const uint64_t el = uni_u64(row[EQ_EL]);
      sumY += y;
      n0 += nj;
#pragma unroll
      for (int k = 0; k < MM; ++k) {
        const int ak = (int)((el >> (8 * k)) & 0xffu);
        if (ak != 0) b0[k] = fma((double)ak, nj, b0[k]);
      }
    }
    const double rsum = 1.0 / sumY;
    n0 *= rsum;
    uint32_t pres = 0;
#pragma unroll
    for (int k = 0; k < MM; ++k) {
      b0[k] *= rsum;
      pres |= (b0[k] > 0.0 ? 1u : 0u) << k;
    }
    const double lnT0 = log(T0), rT0 = 1.0 / T0, lnP0 = log(P0 * (1.0 / PATM));
    double h0 = 0.0, s0 = 0.0;  // H0 / (R T0), S0 / R per gram
    int nact = 0;
    for (int j = 0; j < KK; ++j) {
      const double* row = tab + j * EQ_ROW;
      const double nj = fmax(Yg[j], 0.0) / row[EQ_WT] * rsum;
      double C, H, S;
      nasa7(row, T0, lnT0, rT0, C, H, S);
      h0 = fma(nj, H, h0);
      if (nj > 0.0) s0 = fma(nj, S - log(nj / n0) - lnP0, s0);
      nact += (uni_mask(row[EQ_MASK]) & ~pres) == 0u ? 1 : 0;
    }
    const double V1 = n0 * RU * T0 / P0;   // cm3/g
    const double H1 = h0 * RU * T0;        // erg/g
    const double U1 = H1 - n0 * RU * T0;
    // V held and P free (every V option but 4, P and V): P starts from the ideal gas law
    const bool hasV = (k1 == K_V || k2 == K_V) && k1 != K_P;
    const bool isJ = k2 == K_J;
    // ------------------------------------------------------------ cold start
    double nu = EQ_LN_N_START;
    double th = k1 == K_T ? lnT0 : log(EQ_T_START);
    double vr = isJ ? a.cj_start : 1.0;
    double lnV = log(vr * V1);
    double p = hasV ? nu + th + EQ_LN_RU_PATM - lnV : lnP0;
    bool active = valid && opt >= 1 && opt <= 10 && T0 > 0.0 && P0 > 0.0 && sumY > 0.0;
    int status = active ? -1 : CKMI_RUN_EQ_NOT_CONVERGED;
    if (valid) {
      const double y0 = nu - log((double)(nact > 0 ? nact : 1));
      for (int j = 0; j < KK; ++j) {
        wy[(size_t)j * stride] = y0;
        wd[(size_t)j * stride] = 0.0;
      }
    }
    double lam = 0.0;
    int iters = 0, it_in = 0, kout = 0;
    double lo = a.cj_vlo, hi = a.cj_vhi, vp = 0.0, gp = 0.0;

    // ------------------------------------------------------------ Newton iterations, one per trip
    while (__any(active)) {
      if (active) {
        const double T = exp(th), nn = exp(nu), P = PATM * exp(p), rT = 1.0 / T;
        double A[MM * (MM + 1) / 2], an[MM], anH[MM], anm[MM];
#pragma unroll
        for (int k = 0; k < MM * (MM + 1) / 2; ++k) A[k] = 0.0;
#pragma unroll
        for (int k = 0; k < MM; ++k) an[k] = anH[k] = anm[k] = 0.0;
        double sn = 0.0, snH = 0.0, snm = 0.0, snC = 0.0, snHH = 0.0, snHm = 0.0, snmm = 0.0;
        // pass 1: apply the pending correction, then the sums of the reduced system
        // (the next species' values are loaded before this one's are stored: one species of latency hidden)
        double y_nx = wy[0], d_nx = wd[0];
        for (int j = 0; j < KK; ++j) {
          const double* row = tab + j * EQ_ROW;
          const size_t o = (size_t)j * stride;
          const bool act = (uni_mask(row[EQ_MASK]) & ~pres) == 0u;
          const uint64_t el = uni_u64(row[EQ_EL]);
          const double y = fmax(fma(lam, d_nx, y_nx), nu - 700.0);
          if (j + 1 < KK) {
            y_nx = wy[o + stride];
            d_nx = wd[o + stride];
          }
          double C, H, S;
          nasa7(row, T, th, rT, C, H, S);
          const double nj = act ? exp(y) : 0.0;
          const double m = act ? H - S + y - nu + p : 0.0;
          wy[o] = y;
          wn[o] = nj;
          const double nH = nj * H, nm = nj * m;
          sn += nj;
          snH += nH;
          snm += nm;
          snC = fma(nj, C, snC);
          snHH = fma(nH, H, snHH);
          snHm = fma(nH, m, snHm);
          snmm = fma(nm, m, snmm);
#pragma unroll
          for (int k = 0; k < MM; ++k) {
            const int ak = (int)((el >> (8 * k)) & 0xffu);
            if (ak != 0) {  // wave-uniform
              const double t = (double)ak * nj;
              an[k] += t;
              anH[k] = fma(t, H, anH[k]);
              anm[k] = fma(t, m, anm[k]);
#pragma unroll
              for (int i = 0; i <= k; ++i) {
                const int ai = (int)((el >> (8 * i)) & 0xffu);
                if (ai != 0) A[k * (k + 1) / 2 + i] = fma(t, (double)ai, A[k * (k + 1) / 2 + i]);
              }
            }
          }
        }
        // the reduced system: columns pi_0..pi_MM-1, d nu, d theta, d p, two right-hand sides
        double M[N][N + 2];
#pragma unroll
        for (int r = 0; r < N; ++r)
#pragma unroll
          for (int c = 0; c < N + 2; ++c) M[r][c] = 0.0;
#pragma unroll
        for (int k = 0; k < MM; ++k) {
#pragma unroll
          for (int i = 0; i < MM; ++i) M[k][i] = i <= k ? A[k * (k + 1) / 2 + i] : A[i * (i + 1) / 2 + k];
          if (!((pres >> k) & 1u)) M[k][k] = 1.0;  // absent element: identity row
          M[k][INU] = an[k];
          M[k][IP] = -an[k];
          M[k][ITH] = anH[k];
          M[k][N] = b0[k] - an[k] + anm[k];
          M[MM][k] = an[k];
        }
        M[MM][INU] = sn - nn;
        M[MM][IP] = -sn;
        M[MM][ITH] = snH;
        M[MM][N] = nn - sn + snm;
        const double lnVc = nu + th + EQ_LN_RU_PATM - p;  // ln(n R T / P)
        const double dV = lnV - lnVc;
        // first option row: T, P or V held
        M[MM + 1][INU] = k1 == K_V ? 1.0 : 0.0;
        M[MM + 1][ITH] = k1 == K_P ? 0.0 : 1.0;
        M[MM + 1][IP] = k1 == K_V ? -1.0 : (k1 == K_P ? 1.0 : 0.0);
        M[MM + 1][N] = k1 == K_V ? dV : 0.0;
        M[MM + 1][N + 1] = k1 == K_V ? 1.0 : 0.0;
        // second option row: P or V held, or H / U / S / the Hugoniot with a weight w_j
        if (k2 == K_P) {
          M[MM + 2][IP] = 1.0;
        } else if (k2 == K_V) {
          M[MM + 2][INU] = 1.0;
          M[MM + 2][ITH] = 1.0;
          M[MM + 2][IP] = -1.0;
          M[MM + 2][N] = dV;
          M[MM + 2][N + 1] = 1.0;
        } else {
          const double RT = RU * T;
          // weights: H: w = H_j; U: w = H_j - 1; S: w = H_j - m_j - 1
          const double cm = k2 == K_S ? 1.0 : 0.0, c1 = (k2 == K_U || k2 == K_S) ? 1.0 : 0.0;
#pragma unroll
          for (int k = 0; k < MM; ++k) M[MM + 2][k] = anH[k] - cm * anm[k] - c1 * an[k];
          const double s1 = k2 == K_S ? snH - snm : snH - c1 * sn;
          const double swH = snHH - cm * snHm - c1 * snH;
          const double swm = snHm - cm * snmm - c1 * snm;
          const double tt = k2 == K_U ? snC - sn : snC;
          double res;
          if (k2 == K_U) res = U1 / RT - (snH - sn);
          else if (k2 == K_S) res = s0 - (snH - snm);
          else res = H1 / RT - snH;
          double cnu = s1, cth = tt + swH, cp = -s1;
          if (k2 == K_J) {
            const double Vc = exp(lnVc);
            const double cc1 = 0.5 * (P * V1 / RT + nn), cc2 = 0.5 * (nn - P0 * Vc / RT);
            cnu -= cc2;
            cth -= cc2;
            cp -= cc1 - cc2;
            res += 0.5 * (P - P0) * (V1 + Vc) / RT;
          }
          M[MM + 2][INU] = cnu;
          M[MM + 2][ITH] = cth;
          M[MM + 2][IP] = cp;
          M[MM + 2][N] = res + swm;
        }
        double x[N], dpV;
        solve2<N>(M, x, dpV);
        const double dnu = x[INU], dth = x[ITH], dp = x[IP];
        // pass 2: the species corrections, the damping factor and the convergence measure
        double amax = fmax(5.0 * fabs(dth), fmax(5.0 * fabs(dnu), 5.0 * fabs(dp)));
        double lim = 1.0, cmax = 0.0;
        const double d0 = dnu - dp;
        double n_nx = wn[0];
        y_nx = wy[0];
        for (int j = 0; j < KK; ++j) {
          const double* row = tab + j * EQ_ROW;
          const size_t o = (size_t)j * stride;
          const bool act = (uni_mask(row[EQ_MASK]) & ~pres) == 0u;
          const uint64_t el = uni_u64(row[EQ_EL]);
          const double y = y_nx, nj = n_nx;
          if (j + 1 < KK) {
            y_nx = wy[o + stride];
            n_nx = wn[o + stride];
          }
          double C, H, S;
          nasa7(row, T, th, rT, C, H, S);
          double dy = d0 - (H - S + y - nu + p);  // - m_j, as pass 1 formed it
#pragma unroll
          for (int k = 0; k < MM; ++k) {
            const int ak = (int)((el >> (8 * k)) & 0xffu);
            if (ak != 0) dy = fma((double)ak, x[k], dy);
          }
          dy = act ? fma(H, dth, dy) : 0.0;
          wd[o] = dy;
          const double lnx = y - nu;
          const double ady = fabs(dy);
          if (act) {
            if (lnx > -18.42) amax = fmax(amax, ady);
            else if (dy > 0.0) lim = fmin(lim, fabs((-lnx - 9.212) / (dy - dnu)));
            cmax = fmax(cmax, nj * ady);
          }
        }
        lam = fmin(fmin(1.0, 2.0 / fmax(amax, 1e-300)), lim);
        const double conv = fmax(fmax(cmax / sn, fabs(dnu)), fmax(fabs(dth), fabs(dp)));
        nu = fma(lam, dnu, nu);
        th = fma(lam, dth, th);
        p = fma(lam, dp, p);
        ++iters;
        ++it_in;
        const bool done = lam == 1.0 && conv <= a.tol;
        if (!done) {
          if (it_in >= a.max_iter) {
            status = CKMI_RUN_EQ_NOT_CONVERGED;
            active = false;
          }
        } else if (!isJ) {
          status = CKMI_RUN_OK;
          active = false;
        } else {
          // Chapman-Jouguet: one step of the bracketed secant iteration on g = d ln D^2 / d ln V along the
          // Hugoniot, with d p / d ln V from the second right-hand side
          const double Pn = PATM * exp(p);
          const double g = Pn / (Pn - P0) * dpV + vr / (1.0 - vr);
          if (g < 0.0) lo = vr;
          else hi = vr;
          double vn = kout == 0 ? (g < 0.0 ? vr + 0.05 : vr - 0.05) : vr - g * (vr - vp) / (g - gp);
          if (!(vn > lo && vn < hi)) vn = 0.5 * (lo + hi);
          ++kout;
          if (fabs(vn - vr) <= a.cj_tol) {
            // bisection towards an end of the bracket stops within 2 cj_tol of it: no interior minimum
            const bool ok = vr > a.cj_vlo + 4.0 * a.cj_tol && vr < a.cj_vhi - 4.0 * a.cj_tol;
            status = ok ? CKMI_RUN_OK : CKMI_RUN_EQ_NOT_CONVERGED;
            active = false;
          } else if (kout >= a.cj_iter) {
            status = CKMI_RUN_EQ_NOT_CONVERGED;
            active = false;
          } else {
            vp = vr;
            gp = g;
            vr = vn;
            lnV = log(vn * V1);
            it_in = 0;
          }
        }
      }
    }
    // ------------------------------------------------------------ the returned state
    if (valid) {
      double* __restrict__ Yq = a.Yeq + (size_t)s * KK;
      const bool ran = iters > 0;
      double sum = 0.0;
      for (int j = 0; j < KK; ++j) {
        const double* row = tab + j * EQ_ROW;
        const size_t o = (size_t)j * stride;
        const bool act = (uni_mask(row[EQ_MASK]) & ~pres) == 0u;
        const double y = fmax(fma(lam, wd[o], wy[o]), nu - 700.0);
        const double yj = ran ? (act ? exp(y) * row[EQ_WT] : 0.0) : fmax(Yg[j], 0.0);
        Yq[j] = yj;
        sum += yj;
      }
      const double rs = sum > 0.0 ? 1.0 / sum : 0.0;
      for (int j = 0; j < KK; ++j) Yq[j] *= rs;
      // a held temperature or pressure comes back as given, bit for bit
      const double Tq = ran && k1 != K_T ? exp(th) : T0;
      const double Pq = ran && k1 != K_P && k2 != K_P ? PATM * exp(p) : P0;
      a.Teq[s] = Tq;
      a.Peq[s] = Pq;
      double D = 0.0, snd = 0.0;
      if (isJ && ran) {
        const double Vq = exp(nu + th + EQ_LN_RU_PATM - p);
        D = V1 * sqrt((Pq - P0) / (V1 - Vq));
        snd = D * Vq / V1;
      }
      a.det[s] = D;
      a.sound[s] = snd;
      a.stats[(size_t)CKMI_EQ_NSTAT * s + CKMI_EQ_STAT_ITER] = iters;
      a.stats[(size_t)CKMI_EQ_NSTAT * s + CKMI_EQ_STAT_STATUS] = status;
      a.stats[(size_t)CKMI_EQ_NSTAT * s + CKMI_EQ_STAT_CJ_ITER] = kout;
      a.stats[(size_t)CKMI_EQ_NSTAT * s + 3] = 0;
    }
  }
}

std::mutex g_tab_mu;

// The per-species table, built once per mechanism from its device image (NASA-7 coefficients, molar
// masses and the packed element counts of the corrector's element projection).
int equil_table(const ckmi_mech* cm) {
  std::lock_guard<std::mutex> lock(g_tab_mu);
  if (cm->eq_tab) return CKMI_OK;
  ckmi_mech* m = const_cast<ckmi_mech*>(cm);
  const MechImage& I = m->img;
  std::vector<char> blob((size_t)I.bytes);
  CKMI_HIP_CHECK(hipMemcpy(blob.data(), I.blob, blob.size(), hipMemcpyDeviceToHost));
  const double* th = (const double*)(blob.data() + I.o_th);
  const double* wt = (const double*)(blob.data() + I.o_wt);
  const uint64_t* el = (const uint64_t*)(blob.data() + I.o_e2t + 8 * E2T_N);
  const int KK = m->KK, KKp = I.KKp;
  std::vector<double> tab((size_t)KK * EQ_ROW, 0.0);
  for (int k = 0; k < KK; ++k) {
    double* row = tab.data() + (size_t)k * EQ_ROW;
    row[EQ_TMID] = th[k];
    for (int c = 0; c < 14; ++c) row[EQ_LOW + c] = th[(size_t)(1 + c) * KKp + k];
    row[EQ_WT] = wt[k];
    uint64_t mask = 0;
    for (int e = 0; e < m->npe; ++e) mask |= (uint64_t)(((el[k] >> (8 * e)) & 0xffu) != 0) << e;
    memcpy(&row[EQ_EL], &el[k], 8);
    memcpy(&row[EQ_MASK], &mask, 8);
  }
  void* p = nullptr;
  CKMI_HIP_CHECK(hipMalloc(&p, tab.size() * sizeof(double)));
  m->allocs.push_back(p);
  CKMI_HIP_CHECK(hipMemcpy(p, tab.data(), tab.size() * sizeof(double), hipMemcpyHostToDevice));
  m->eq_mm = m->npe;
  m->eq_tab = (const double*)p;
  return CKMI_OK;
}

template <int MM>
int launch_equil(const ckmi_mech* m, EqArgs a, hipStream_t st) {
  const size_t lds = (size_t)a.KK * EQ_ROW * sizeof(double);
  int ncu = 0, per_cu = 0;
  CKMI_HIP_CHECK(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, m->device));
  if (int rc = raise_lds_limit(m->device, (const void*)equil_kernel<MM>, lds)) return rc;
  CKMI_HIP_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, equil_kernel<MM>, EQ_BLOCK, lds));
  if (per_cu < 1) return set_error(CKMI_ERR_SIZE, "equilibrium kernel does not fit on a CU");
  const int tiles = (a.n + EQ_BLOCK - 1) / EQ_BLOCK;
  const int grid = std::max(1, std::min(ncu * per_cu, tiles));
  const size_t wbytes = 3 * (size_t)a.KK * grid * EQ_BLOCK * sizeof(double);
  StreamWorkspace ws(st);
  if (int rc = ws.alloc(wbytes)) return rc;
  a.ws = ws.take<double>(wbytes);
  hipLaunchKernelGGL((equil_kernel<MM>), dim3(grid), dim3(EQ_BLOCK), lds, st, a);
  CKMI_HIP_CHECK(hipGetLastError());
  return CKMI_OK;
}

}  // namespace

extern "C" {

int ckmi_equil_run(const ckmi_mech* m, const ckmi_equil_cfg* cfg, int32_t n, const int32_t* option, const double* T,
                   const double* P, const double* Y, double* Teq, double* Peq, double* Yeq, double* sound,
                   double* detspeed, int32_t* stats, void* stream) {
  if (!m || !cfg || n < 0) return set_error(CKMI_ERR_ARG, "bad argument");
  if (!(cfg->tol >= 0.0) || cfg->max_iter < 0 || cfg->cj_iter < 0)
    return set_error(CKMI_ERR_ARG, "tol, max_iter and cj_iter must be >= 0 (0: the default)");
  const double vlo = cfg->cj_vlo == 0.0 ? 0.30 : cfg->cj_vlo, vhi = cfg->cj_vhi == 0.0 ? 0.97 : cfg->cj_vhi;
  const double v0 = cfg->cj_start == 0.0 ? 0.60 : cfg->cj_start;
  if (!(vlo > 0.0 && vlo < v0 && v0 < vhi && vhi < 1.0) || !(cfg->cj_tol >= 0.0))
    return set_error(CKMI_ERR_ARG, "the CJ bracket needs 0 < cj_vlo < cj_start < cj_vhi < 1 and cj_tol >= 0");
  if (m->npe < 1)
    return set_error(CKMI_ERR_UNSUPPORTED, "the equilibrium solver needs the element counts of a mechanism with at most " +
                                          std::to_string(CKMI_PROJ_MMAX) + " elements");
  if (n > 0 && (!option || !T || !P || !Y || !Teq || !Peq || !Yeq || !sound || !detspeed || !stats))
    return set_error(CKMI_ERR_ARG, "every input and output array is required");
  if (n == 0) return CKMI_OK;
  if (int rc = equil_table(m)) return rc;
  EqArgs a{};
  a.n = n;
  a.KK = m->KK;
  a.tab = m->eq_tab;
  a.option = option;
  a.T = T;
  a.P = P;
  a.Y = Y;
  a.Teq = Teq;
  a.Peq = Peq;
  a.Yeq = Yeq;
  a.sound = sound;
  a.det = detspeed;
  a.stats = stats;
  a.tol = cfg->tol == 0.0 ? 1e-12 : cfg->tol;
  a.max_iter = cfg->max_iter == 0 ? 200 : cfg->max_iter;
  a.cj_vlo = vlo;
  a.cj_vhi = vhi;
  a.cj_start = v0;
  a.cj_tol = cfg->cj_tol == 0.0 ? 1e-9 : cfg->cj_tol;
  a.cj_iter = cfg->cj_iter == 0 ? 40 : cfg->cj_iter;
  const hipStream_t st = (hipStream_t)stream;
  switch (m->eq_mm) {
    case 1: return launch_equil<1>(m, a, st);
    case 2: return launch_equil<2>(m, a, st);
    case 3: return launch_equil<3>(m, a, st);
    case 4: return launch_equil<4>(m, a, st);
    case 5: return launch_equil<5>(m, a, st);
    case 6: return launch_equil<6>(m, a, st);
    case 7: return launch_equil<7>(m, a, st);
    case 8: return launch_equil<8>(m, a, st);
    default: return set_error(CKMI_ERR_UNSUPPORTED, "more than 8 elements");
  }
}

}  // extern "C"
