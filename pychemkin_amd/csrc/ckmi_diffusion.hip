// ckmi_diffusion.hip -- binary, mixture-averaged and ordinary multicomponent diffusion coefficients on gfx950.
//
// The reference's closed library evaluates them on demand from the transport file preprocessed by
// KINPreProcess (itran = 1): KINGetDiffusionCoeffs (chemistry.py:1410-1470, mixture.py:1910),
// KINGetMixtureDiffusionCoeffs (mixture.py:2015) and KINGetOrdinaryDiffusionCoeffs (mixture.py:2066).
// Restated method (TRANFIT / TRANLIB), on the ln-T cubics of ln D_jk at 1 atm from ckmi_diffusion_fit
// (ckmi_transport.hip):
//
//   binary             D_jk = exp(cubic_jk(ln T)) 1 atm / P
//   mole fractions     X = (X+ + 1e-12) / sum (X+ + 1e-12), X+ from max(Y, 0); Wbar = sum X_k W_k
//                      (the floor keeps the pure-species limit finite, as in Chemkin's flame codes)
//   mixture-averaged   D_km = sum_{j != k} X_j W_j / (Wbar sum_{j != k} X_j / D_jk)
//   multicomponent     L_ij = 16 T / (25 P) sum_k X_k / (W_i D_ik) {W_j X_j (1 - d_ik) - W_i X_i (d_ij - d_jk)}
//                           = 16 T / (25 P) X_j (W_j S_i / W_i + X_i / D_ij) off the diagonal, S_i = sum_{k != i} X_k / D_ik,
//                      and L_ii = 0 identically (the three terms cancel), so p = L^-1 needs row pivoting;
//                      D_ij = X_i 16 T / (25 P) Wbar / W_j (p_ij - p_ii)  (Dixon-Lewis first order, MCMDIF)
//
// Kernels and what bounds them:
//   binary_diffusion_kernel    one output element per thread: HBM writes, KK^2 x 8 B per state;
//   mixture_diffusion_kernel   one state per lane, its X column in LDS ([KK][block], conflict-free), the
//                              (k, j) fit rows by wave-uniform scalar loads, D_jk evaluated inside the KK^2
//                              loop (the binary matrix never goes to HBM): FP64 exp, KK^2 per state;
//   mc_wave_kernel<NC>         KK <= 64: one wave per state, lane = row, the row of L and then of L^-1 in NC
//                              doubles per lane (2 NC VGPRs), in-place Gauss-Jordan with the pivot row found by a
//                              wave max reduction and broadcast by readlane; rows never move (each lane records
//                              the column it was the pivot of), the permutation is undone through an LDS
//                              staging of L^-1 from which D goes to HBM coalesced: FP64 VALU,
//                              KK x NC FMAs + 2 readlanes each per state;
//   mc_assemble_kernel, ckmi_lu_factor_batched, mc_finish_kernel
//                              64 < KK <= CKMI_LU_NMAX: one workgroup per state; L goes to a workspace, is
//                              factored by the pivoted blocked LU of ckmi_lu.hip, and thread j of the finishing
//                              kernel solves for column j of the identity in place in D (coalesced across the
//                              threads, the factors by wave-uniform loads): L2 traffic of the substitutions,
//                              KK^3 x 16 B per state.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <algorithm>
#include <string>

#include "../../include/ckmi.h"
#include "ckmi_internal.hpp"
#include "ckmi_transport.hpp"

namespace {

constexpr int WAVE = 64;
constexpr int BIG_BS = 256;        // threads of the workgroup-per-state kernels (>= CKMI_LU_NMAX)
constexpr double XFLOOR = 1e-12;   // mole-fraction floor
using ckmi_tran::P_ATM;

static_assert(BIG_BS >= CKMI_LU_NMAX, "one thread per column in the workgroup kernels");

int fail(int code, const std::string& msg) { return ckmi::set_error(code, msg); }

__device__ __forceinline__ double cubic(const double* __restrict__ a, double x) {
  return fma(x, fma(x, fma(x, a[3], a[2]), a[1]), a[0]);
}

__global__ void binary_diffusion_kernel(int KK, int n, const double* __restrict__ dfits, const double* __restrict__ T,
                                        const double* __restrict__ P, double* __restrict__ D) {
  const size_t kk2 = (size_t)KK * KK, total = kk2 * (size_t)n;
  for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
    const size_t s = idx / kk2, e = idx - s * kk2;
    D[idx] = exp(cubic(dfits + 4 * e, log(T[s]))) * (P_ATM / P[s]);
  }
}

// one state per lane; dynamic LDS: X [KK][blockDim]
__global__ void mixture_diffusion_kernel(int KK, int n, const double* __restrict__ dfits, const double* __restrict__ wt,
                                         const double* __restrict__ T, const double* __restrict__ P,
                                         const double* __restrict__ Y, double* __restrict__ D) {
  extern __shared__ double md_lds[];
  const int bs = blockDim.x, t = threadIdx.x;
  const int i = blockIdx.x * bs + t;
  const bool live = i < n;
  const int ii = live ? i : 0;
  double* Xs = md_lds + t;  // Xs[k * bs]
  const double x = log(T[ii]);
  const double pr = P[ii] / P_ATM;  // 1 / D_jk(P) = exp(-cubic) P / 1 atm
  double sx = 0.0;
  for (int k = 0; k < KK; ++k) {
    const double xk = fmax(Y[(size_t)k * n + ii], 0.0) / wt[k];  // negative traces count as 0
    Xs[k * bs] = xk;
    sx += xk;
  }
  const double inv = sx > 0.0 ? 1.0 / sx : 0.0;
  double st = 0.0;
  for (int k = 0; k < KK; ++k) {
    const double xt = fma(Xs[k * bs], inv, XFLOOR);
    Xs[k * bs] = xt;
    st += xt;
  }
  double wbar = 0.0;
  for (int k = 0; k < KK; ++k) {
    const double xt = Xs[k * bs] / st;
    Xs[k * bs] = xt;
    wbar = fma(xt, wt[k], wbar);
  }
  for (int k = 0; k < KK; ++k) {
    const double* fk = dfits + 4 * (size_t)k * KK;
    double num = 0.0, den = 0.0;
    for (int j = 0; j < KK; ++j) {
      if (j == k) continue;
      const double xj = Xs[j * bs];
      num = fma(xj, wt[j], num);
      den = fma(xj, exp(-cubic(fk + 4 * j, x)), den);
    }
    // a single-species mechanism has no other species to diffuse into: its self-diffusion coefficient
    const double d = den > 0.0 ? num / (wbar * den * pr) : exp(cubic(fk + 4 * k, x)) / pr;
    if (live) D[(size_t)k * n + i] = d;
  }
}

// bitwise the same on every lane (each butterfly level adds the same two partial sums, commutatively)
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int m = 1; m < WAVE; m <<= 1) v += __shfl_xor(v, m, WAVE);
  return v;
}
__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
  for (int m = 1; m < WAVE; m <<= 1) v = fmax(v, __shfl_xor(v, m, WAVE));
  return v;
}
__device__ __forceinline__ double bcast(double v, int lane) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), lane);
  const int hi = __builtin_amdgcn_readlane(__double2hiint(v), lane);
  return __hiloint2double(hi, lo);
}

// One wave per state, KK <= NC <= 64; lane i < KK holds row i.  Dynamic LDS: the staging of L^-1 [KK][KK | 1],
// then X [64], W [64] and the pivot lane of every column [64].
template <int NC>
__global__ __launch_bounds__(WAVE) void mc_wave_kernel(int KK, int n, const double* __restrict__ dfits,
                                                       const double* __restrict__ wt, const double* __restrict__ T,
                                                       const double* __restrict__ P, const double* __restrict__ Y,
                                                       double* __restrict__ D, int* __restrict__ info) {
  extern __shared__ double mc_lds[];
  const int lane = threadIdx.x;
  const int s = blockIdx.x;
  const int LD = KK | 1;  // odd row stride: the permuted column stores of a wave spread over the banks
  double* S = mc_lds;
  double* Xs = S + KK * LD;
  double* Ws = Xs + WAVE;
  int* rcs = reinterpret_cast<int*>(Ws + WAVE);
  const bool real = lane < KK;
  const int li = real ? lane : 0;
  const double Ts = T[s], Ps = P[s];
  const double w = wt[li];
  const double xk = real ? fmax(Y[(size_t)li * n + s], 0.0) / w : 0.0;  // negative traces count as 0
  const double sx = wave_sum(xk);
  double xt = real ? fma(xk, sx > 0.0 ? 1.0 / sx : 0.0, XFLOOR) : 0.0;
  xt /= wave_sum(xt);
  const double wbar = wave_sum(xt * w);
  Xs[lane] = xt;
  Ws[lane] = w;
  __syncthreads();
  const double x = log(Ts);
  const double cf = 16.0 * Ts / (25.0 * Ps);
  const double pr = Ps / P_ATM;
  const double* fr = dfits + 4 * (size_t)li * KK;
  double a[NC];
  double Si = 0.0;
#pragma unroll
  for (int k = 0; k < NC; ++k) {  // a[k] = 1 / D_ik, S_i = sum_{k != i} X_k / D_ik
    double r = 0.0;
    if (k < KK) r = (real && k != lane) ? exp(-cubic(fr + 4 * k, x)) * pr : 0.0;
    a[k] = r;
    Si = fma(Xs[k], r, Si);
  }
  const double sw = Si / w;
#pragma unroll
  for (int j = 0; j < NC; ++j) {
    double v = 0.0;
    if (j < KK) v = (real && j != lane) ? cf * Xs[j] * fma(Ws[j], sw, xt * a[j]) : 0.0;
    a[j] = v;
  }
  // in-place Gauss-Jordan, partial pivoting over the lanes that have not been a pivot row yet
  bool used = !real;
  int mycol = -1;
  int zinfo = 0;
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    if (c < KK) {  // (wave-uniform)
      const double f = a[c];
      const double v = used ? -1.0 : fabs(f);
      const double maxv = wave_max(v);
      const uint64_t cand = __ballot(!used && v == maxv);
      const int pl = __builtin_amdgcn_readfirstlane(cand ? (int)__ffsll((unsigned long long)cand) - 1 : 0);
      const bool ok = maxv > 0.0;
      zinfo = (!ok && zinfo == 0) ? c + 1 : zinfo;
      const double rp = ok ? 1.0 / bcast(f, pl) : 0.0;
      const bool isp = lane == pl;
      used = used || isp;
      mycol = isp ? c : mycol;
      if (lane == 0) rcs[c] = pl;
      if (isp) {
#pragma unroll
        for (int cc = 0; cc < NC; ++cc) a[cc] *= rp;
      }
      a[c] = isp ? rp : 0.0;
      const double fe = isp ? 0.0 : f;
#pragma unroll
      for (int cc = 0; cc < NC; ++cc) a[cc] = fma(-fe, bcast(a[cc], pl), a[cc]);
    }
  }
  __syncthreads();
  // the lane that was the pivot of column i holds row i of (P L)^-1 = L^-1 P^T: its register c is L^-1[i][rcs[c]]
  if (mycol >= 0) {
#pragma unroll
    for (int c = 0; c < NC; ++c)
      if (c < KK) S[mycol * LD + rcs[c]] = a[c];
  }
  __syncthreads();
  const double sc = cf * wbar;
  double* Ds = D + (size_t)s * KK * KK;
  for (int idx = lane; idx < KK * KK; idx += WAVE) {
    const int i = idx / KK, j = idx - i * KK;
    Ds[idx] = i == j ? 0.0 : Xs[i] * sc / Ws[j] * (S[i * LD + j] - S[i * LD + i]);
  }
  if (lane == 0) info[s] = zinfo;
}

// Workgroup path, step 1: thread i < KK writes row i of L to Lw [KK][KK] and X (then Wbar) to xw [KK + 1].
__global__ __launch_bounds__(BIG_BS) void mc_assemble_kernel(int KK, int n, int s0, const double* __restrict__ dfits,
                                                             const double* __restrict__ wt, const double* __restrict__ T,
                                                             const double* __restrict__ P, const double* __restrict__ Y,
                                                             double* __restrict__ Lw, double* __restrict__ xw) {
  __shared__ double Xs[CKMI_LU_NMAX];
  const int i = threadIdx.x;
  const int s = s0 + blockIdx.x;
  const bool real = i < KK;
  const double w = real ? wt[i] : 1.0;
  if (real) Xs[i] = fmax(Y[(size_t)i * n + s], 0.0) / w;
  __syncthreads();
  // every thread sums the KK entries itself, in the same order: the same sx, st and Wbar on all of them
  double sx = 0.0;
  for (int k = 0; k < KK; ++k) sx += Xs[k];
  const double inv = sx > 0.0 ? 1.0 / sx : 0.0;
  double st = 0.0;
  for (int k = 0; k < KK; ++k) st += fma(Xs[k], inv, XFLOOR);
  const double xt = real ? fma(Xs[i], inv, XFLOOR) / st : 0.0;
  __syncthreads();
  if (real) Xs[i] = xt;
  __syncthreads();
  if (!real) return;
  double wbar = 0.0;
  for (int k = 0; k < KK; ++k) wbar = fma(Xs[k], wt[k], wbar);
  double* xs = xw + (size_t)blockIdx.x * (KK + 1);
  xs[i] = xt;
  if (i == 0) xs[KK] = wbar;
  const double Ts = T[s], Ps = P[s];
  const double x = log(Ts);
  const double cf = 16.0 * Ts / (25.0 * Ps);
  const double pr = Ps / P_ATM;
  const double* fr = dfits + 4 * (size_t)i * KK;
  double* Li = Lw + ((size_t)blockIdx.x * KK + i) * KK;
  double Si = 0.0;
  for (int k = 0; k < KK; ++k) {  // 1 / D_ik parked in the row, read back by this thread below
    const double r = k != i ? exp(-cubic(fr + 4 * k, x)) * pr : 0.0;
    Li[k] = r;
    Si = fma(Xs[k], r, Si);
  }
  const double sw = Si / w;
  for (int j = 0; j < KK; ++j) Li[j] = j != i ? cf * Xs[j] * fma(wt[j], sw, xt * Li[j]) : 0.0;
}

// Workgroup path, step 3: from the factors P L U of step 2, thread j < KK solves L x = e_j in place in column j
// of D (dgetrs on one column of the identity), then D_ij = X_i 16 T / (25 P) Wbar / W_j (x_ij - x_ii).
__global__ __launch_bounds__(BIG_BS) void mc_finish_kernel(int KK, int s0, const double* __restrict__ LUw,
                                                           const int* __restrict__ ipiv, const double* __restrict__ xw,
                                                           const double* __restrict__ wt, const double* __restrict__ T,
                                                           const double* __restrict__ P, double* D) {
  __shared__ double diag[CKMI_LU_NMAX];
  const int j = threadIdx.x;
  const int s = s0 + blockIdx.x;
  const double* LU = LUw + (size_t)blockIdx.x * KK * KK;
  const int* piv = ipiv + (size_t)blockIdx.x * KK;
  const double* xs = xw + (size_t)blockIdx.x * (KK + 1);
  double* Ds = D + (size_t)s * KK * KK;
  if (j < KK) {
    int pos = j;  // the row of the 1 of P e_j after the interchanges in order (dlaswp)
    for (int i = 0; i < KK; ++i) {
      const int p = piv[i];
      pos = pos == i ? p : (pos == p ? i : pos);
    }
    for (int i = 0; i < KK; ++i) {  // unit-lower L y = P e_j
      double acc = i == pos ? 1.0 : 0.0;
      for (int k = 0; k < i; ++k) acc = fma(-LU[(size_t)i * KK + k], Ds[(size_t)k * KK + j], acc);
      Ds[(size_t)i * KK + j] = acc;
    }
    for (int i = KK - 1; i >= 0; --i) {  // U x = y
      double acc = Ds[(size_t)i * KK + j];
      for (int k = i + 1; k < KK; ++k) acc = fma(-LU[(size_t)i * KK + k], Ds[(size_t)k * KK + j], acc);
      Ds[(size_t)i * KK + j] = acc / LU[(size_t)i * KK + i];
    }
  }
  __syncthreads();
  if (j < KK) diag[j] = Ds[(size_t)j * KK + j];
  __syncthreads();
  const double sc = 16.0 * T[s] / (25.0 * P[s]) * xs[KK];
  for (int idx = j; idx < KK * KK; idx += BIG_BS) {
    const int i = idx / KK, c = idx - i * KK;
    Ds[idx] = i == c ? 0.0 : xs[i] * sc / wt[c] * (Ds[idx] - diag[i]);
  }
}

template <int NC>
hipError_t launch_mc_wave(const ckmi_transport* t, int n, const double* T, const double* P, const double* Y, double* D,
                          int* info, hipStream_t st) {
  const int KK = t->KK;
  const size_t lds = sizeof(double) * ((size_t)KK * (KK | 1) + 2 * WAVE) + sizeof(int) * WAVE;
  hipLaunchKernelGGL(mc_wave_kernel<NC>, dim3(n), dim3(WAVE), lds, st, KK, n, t->dfits, t->wt, T, P, Y, D, info);
  return hipGetLastError();
}

}  // namespace

extern "C" {

int ckmi_binary_diffusion(const ckmi_transport* t, int32_t n, const double* T, const double* P, double* D,
                          void* stream) {
  if (!t || n < 0) return fail(CKMI_ERR_ARG, "ckmi_binary_diffusion: bad argument");
  if (!t->dfits) return fail(CKMI_ERR_ARG, "ckmi_binary_diffusion: no diffusion fits (ckmi_transport_set_diffusion)");
  if (n == 0) return CKMI_OK;  // (an empty batch has no arrays)
  if (!T || !P || !D) return fail(CKMI_ERR_ARG, "ckmi_binary_diffusion: null array");
  const int bs = 256;
  const size_t total = (size_t)t->KK * t->KK * (size_t)n;
  const size_t grid = std::min<size_t>((total + bs - 1) / bs, (size_t)1 << 20);
  hipLaunchKernelGGL(binary_diffusion_kernel, dim3((unsigned)grid), dim3(bs), 0, (hipStream_t)stream, t->KK, n, t->dfits,
                     T, P, D);
  if (hipGetLastError() != hipSuccess) return fail(CKMI_ERR_HIP, "binary_diffusion_kernel launch failed");
  return CKMI_OK;
}

int ckmi_mixture_diffusion(const ckmi_transport* t, int32_t n, const double* T, const double* P, const double* Y,
                           double* D, void* stream) {
  if (!t || n < 0) return fail(CKMI_ERR_ARG, "ckmi_mixture_diffusion: bad argument");
  if (!t->dfits) return fail(CKMI_ERR_ARG, "ckmi_mixture_diffusion: no diffusion fits (ckmi_transport_set_diffusion)");
  if (n == 0) return CKMI_OK;
  if (!T || !P || !Y || !D) return fail(CKMI_ERR_ARG, "ckmi_mixture_diffusion: null array");
  // one wave per block up to 320 species (<= 160 KB of LDS), half a wave above
  const int bs = t->KK <= 320 ? 64 : 32;
  const size_t lds = sizeof(double) * (size_t)t->KK * bs;
  if (lds > 160 * 1024) return fail(CKMI_ERR_UNSUPPORTED, "ckmi_mixture_diffusion: more than 640 species");
  if (lds > 64 * 1024 &&
      hipFuncSetAttribute((const void*)mixture_diffusion_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) !=
          hipSuccess)
    return fail(CKMI_ERR_HIP, "ckmi_mixture_diffusion: LDS attribute failed");
  hipLaunchKernelGGL(mixture_diffusion_kernel, dim3((n + bs - 1) / bs), dim3(bs), lds, (hipStream_t)stream, t->KK, n,
                     t->dfits, t->wt, T, P, Y, D);
  if (hipGetLastError() != hipSuccess) return fail(CKMI_ERR_HIP, "mixture_diffusion_kernel launch failed");
  return CKMI_OK;
}

int ckmi_multicomponent_diffusion(const ckmi_transport* t, int32_t n, const double* T, const double* P,
                                  const double* Y, double* D, int32_t* info, void* stream) {
  if (!t || n < 0) return fail(CKMI_ERR_ARG, "ckmi_multicomponent_diffusion: bad argument");
  if (!t->dfits)
    return fail(CKMI_ERR_ARG, "ckmi_multicomponent_diffusion: no diffusion fits (ckmi_transport_set_diffusion)");
  const int KK = t->KK;
  if (KK > CKMI_LU_NMAX)
    return fail(CKMI_ERR_UNSUPPORTED,
                "ckmi_multicomponent_diffusion: more than " + std::to_string(CKMI_LU_NMAX) + " species");
  if (n == 0) return CKMI_OK;
  if (!T || !P || !Y || !D || !info) return fail(CKMI_ERR_ARG, "ckmi_multicomponent_diffusion: null array");
  hipStream_t st = (hipStream_t)stream;
  if (KK <= WAVE) {
    const hipError_t e = KK <= 16   ? launch_mc_wave<16>(t, n, T, P, Y, D, info, st)
                         : KK <= 32 ? launch_mc_wave<32>(t, n, T, P, Y, D, info, st)
                         : KK <= 48 ? launch_mc_wave<48>(t, n, T, P, Y, D, info, st)
                         : KK <= 56 ? launch_mc_wave<56>(t, n, T, P, Y, D, info, st)
                                    : launch_mc_wave<64>(t, n, T, P, Y, D, info, st);
    if (e != hipSuccess) return fail(CKMI_ERR_HIP, std::string("mc_wave_kernel launch: ") + hipGetErrorString(e));
    return CKMI_OK;
  }
  // workgroup path: L, X and the pivots of up to `chunk` states in a workspace of at most ~256 MB, freed on return
  const size_t kk2 = (size_t)KK * KK;
  const int chunk = (int)std::min<size_t>((size_t)n, std::max<size_t>(1, ((size_t)256 << 20) / (kk2 * sizeof(double))));
  double* Lw = nullptr;
  double* xw = nullptr;
  int* ipiv = nullptr;
  int rc = CKMI_OK;
  if (hipMalloc(&Lw, sizeof(double) * kk2 * chunk) != hipSuccess ||
      hipMalloc(&xw, sizeof(double) * (size_t)(KK + 1) * chunk) != hipSuccess ||
      hipMalloc(&ipiv, sizeof(int) * (size_t)KK * chunk) != hipSuccess)
    rc = fail(CKMI_ERR_HIP, "ckmi_multicomponent_diffusion: workspace allocation failed");
  for (int s0 = 0; rc == CKMI_OK && s0 < n; s0 += chunk) {
    const int cnt = std::min(chunk, n - s0);
    hipLaunchKernelGGL(mc_assemble_kernel, dim3(cnt), dim3(BIG_BS), 0, st, KK, n, s0, t->dfits, t->wt, T, P, Y, Lw, xw);
    if (hipGetLastError() != hipSuccess) {
      rc = fail(CKMI_ERR_HIP, "mc_assemble_kernel launch failed");
      break;
    }
    if (ckmi_lu_factor_batched(cnt, KK, Lw, ipiv, info + s0, stream) != CKMI_OK) {
      rc = fail(CKMI_ERR_HIP, std::string("ckmi_multicomponent_diffusion: ") + ckmi_lu_last_error());
      break;
    }
    hipLaunchKernelGGL(mc_finish_kernel, dim3(cnt), dim3(BIG_BS), 0, st, KK, s0, Lw, ipiv, xw, t->wt, T, P, D);
    if (hipGetLastError() != hipSuccess) rc = fail(CKMI_ERR_HIP, "mc_finish_kernel launch failed");
  }
  // the workspace is in use until the stream has drained
  if (hipStreamSynchronize(st) != hipSuccess && rc == CKMI_OK)
    rc = fail(CKMI_ERR_HIP, "ckmi_multicomponent_diffusion: stream synchronisation failed");
  (void)hipFree(Lw);
  (void)hipFree(xw);
  (void)hipFree(ipiv);
  return rc;
}

}  // extern "C"
