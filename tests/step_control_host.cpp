// step_control_host.cpp -- the straight-line BDF order helpers of ckmi_reactor.hpp against the branch forms they
// replaced, word for word, on the host.  Built and run by tests/test_step_control_host.py (host-only compile; no
// GPU and no Python process is involved, so it can be built with -fsanitize=address,undefined and run directly).
//
// Helpers under test: bdf_rescale, bdf_adjust_order (+1 and -1), dky0_lane, bdf_correct_history (the history
// update zn[j] += l[j] * acor with the parked acor) and bdf_tau_shift.  The reference below restates the loops
// as they were: one conditional access per order, in the order the integrator ran them.
// Cases: every q in 1..5, nst in {0, 1, 2, 20}, seeded random histories, and the values +-0, denormals,
// +-inf and NaN planted in every field the helpers read.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>

#include "../pychemkin_amd/csrc/ckmi_reactor.hpp"

using namespace ckmi;

namespace {

// plain-array history: the same fields as BdfT<ST>, zn as an array
struct HostB {
  double zn[QMAX + 1];
  double ewt, acor, tempv, ftemp, y;
};

// ---------------------------------------------------------------- the branch forms (reference)
void ref_rescale(HostB& b, BdfS& S) {
  double factor = S.eta;
  for (int j = 1; j <= QMAX; ++j) {
    if (j <= S.q) {
      b.zn[j] *= factor;
      factor *= S.eta;
    }
  }
  S.h = S.hscale * S.eta;
  S.hscale = S.h;
}

void ref_adjust_order(HostB& b, BdfS& S, int deltaq) {
  const int q = S.q;
  for (int i = 0; i <= QMAX; ++i) S.l[i] = 0.0;
  S.l[2] = 1.0;
  if (deltaq == 1) {
    double alpha1 = 1.0, prod = 1.0, xiold = 1.0, alpha0 = -1.0, hsum = S.hscale;
    for (int j = 1; j < QMAX; ++j) {
      if (j < q) {
        hsum += S.tau[j + 1];
        const double xi = hsum / S.hscale;
        prod *= xi;
        alpha0 -= 1.0 / (j + 1);
        alpha1 += 1.0 / xi;
        for (int i = QMAX; i >= 2; --i)
          if (i <= j + 2) S.l[i] = S.l[i] * xiold + S.l[i - 1];
        xiold = xi;
      }
    }
    const double A1 = (-alpha0 - alpha1) / prod;
    const double znL = A1 * b.zn[QMAX];
    for (int j = 2; j <= QMAX; ++j)
      if (j <= q) b.zn[j] += S.l[j] * znL;
    for (int j = 1; j <= QMAX; ++j)
      if (j == q + 1) b.zn[j] = znL;
  } else {
    double hsum = 0.0;
    for (int j = 1; j <= QMAX; ++j) {
      if (j <= q - 2) {
        hsum += S.tau[j];
        const double xi = hsum / S.hscale;
        for (int i = QMAX; i >= 2; --i)
          if (i <= j + 2) S.l[i] = S.l[i] * xi + S.l[i - 1];
      }
    }
    double znq = 0.0;
    for (int j = 0; j <= QMAX; ++j)
      if (j == q) znq = b.zn[j];
    for (int j = 2; j <= QMAX; ++j)
      if (j < q) b.zn[j] -= S.l[j] * znq;
  }
}

double ref_dky0(const HostB& b, const BdfS& S, double t) {
  const double sc = (t - S.tn) / S.h;
  double v = 0.0;
  for (int j = QMAX; j >= 0; --j)
    if (j <= S.q) v = b.zn[j] + sc * v;
  return v;
}

// ST_STEP_COMPLETE's history update; qwait is the value after its decrement
void ref_correct_history(HostB& b, const BdfS& S, int qwait) {
  for (int j = 0; j <= QMAX; ++j)
    if (j <= S.q) b.zn[j] += S.l[j] * b.acor;
  if (qwait == 1 && S.q != QMAX) b.zn[QMAX] = b.acor;
}

// ST_STEP_COMPLETE's step-size shift (S.nst already counts the accepted step); returns tau[2] as read after it
double ref_tau_shift(BdfS& S) {
  for (int i = QMAX; i >= 2; --i)
    if (i <= S.q) S.tau[i] = S.tau[i - 1];
  if (S.q == 1 && S.nst > 1) S.tau[2] = S.tau[1];
  S.tau[1] = S.h;
  return S.tau[2];
}

// ---------------------------------------------------------------- inputs
double from_bits(uint64_t u) {
  double d;
  std::memcpy(&d, &u, 8);
  return d;
}
uint64_t bits(double d) {
  uint64_t u;
  std::memcpy(&u, &d, 8);
  return u;
}
const double SPECIAL[] = {0.0,
                          -0.0,
                          from_bits(1ull),                    // smallest denormal
                          -from_bits(1ull),
                          from_bits(0x000fffffffffffffull),   // largest denormal
                          -from_bits(0x0000000123456789ull),
                          from_bits(0x7ff0000000000000ull),   // +inf
                          from_bits(0xfff0000000000000ull),   // -inf
                          from_bits(0x7ff8000000000000ull)};  // NaN
constexpr int NSPECIAL = sizeof(SPECIAL) / sizeof(SPECIAL[0]);

struct Gen {
  std::mt19937_64 r;
  explicit Gen(uint64_t seed) : r(seed) {}
  double unit() { return (double)(r() >> 11) * (1.0 / 9007199254740992.0); }  // [0, 1)
  // a history-like value: either sign, 1e-12 .. 1e3 in magnitude
  double val() {
    const double m = std::exp2(-40.0 + 50.0 * unit());
    return (r() & 1) ? m : -m;
  }
  double pos() { return std::exp2(-30.0 + 30.0 * unit()); }  // a step size
};

// the doubles the helpers read: zn[0..5], acor, l[0..5], tau[0..6], eta, h, hscale, tn
constexpr int NFIELD = 6 + 1 + 6 + 7 + 4;
double* field(HostB& b, BdfS& S, int k) {
  if (k < 6) return &b.zn[k];
  if (k == 6) return &b.acor;
  if (k < 13) return &S.l[k - 7];
  if (k < 20) return &S.tau[k - 13];
  if (k == 20) return &S.eta;
  if (k == 21) return &S.h;
  if (k == 22) return &S.hscale;
  return &S.tn;
}

void fill(Gen& g, HostB& b, BdfS& S, int q, int nst) {
  std::memset(&b, 0, sizeof b);  // padding too: the outputs are compared as words
  std::memset(&S, 0, sizeof S);
  for (int j = 0; j <= QMAX; ++j) b.zn[j] = g.val();
  b.acor = g.val();
  b.ewt = g.pos();
  for (int j = 0; j <= QMAX; ++j) S.l[j] = g.val();
  for (int i = 0; i <= QMAX + 1; ++i) S.tau[i] = g.pos();
  for (int i = 0; i < 6; ++i) S.tq[i] = g.pos();
  S.h = g.pos();
  S.hscale = g.pos();
  S.hprime = g.pos();
  S.eta = 0.1 + 9.9 * g.unit();
  S.tn = g.pos();
  S.q = q;
  S.L = q + 1;
  S.nst = nst;
}

long n_checked = 0, n_bad = 0;
void same(const char* what, const void* a, const void* r, size_t n, int q, int nst, long trial) {
  // Every 8-byte word must be equal, with one allowance: a NaN matches a NaN.  IEEE 754 leaves the sign and
  // payload of an arithmetic NaN open; x86 takes them from the first source operand of the instruction, which
  // for a commutative operation is the compiler's choice (seen here: 7ff8.. against fff8.. for the same sum).
  // The integer fields of BdfS are small counts and never pair up to a NaN pattern.
  ++n_checked;
  bool bad = n % 8 != 0;
  for (size_t w = 0; w + 8 <= n; w += 8) {
    uint64_t x, y;
    std::memcpy(&x, (const char*)a + w, 8);
    std::memcpy(&y, (const char*)r + w, 8);
    const bool xn = (x & 0x7fffffffffffffffull) > 0x7ff0000000000000ull;
    const bool yn = (y & 0x7fffffffffffffffull) > 0x7ff0000000000000ull;
    if (x != y && !(xn && yn)) {
      if (n_bad < 20)
        std::printf("MISMATCH %s q=%d nst=%d trial=%ld word %zu: %016llx != %016llx\n", what, q, nst, trial, w / 8,
                    (unsigned long long)x, (unsigned long long)y);
      bad = true;
    }
  }
  if (bad) ++n_bad;
}

void run_case(const HostB& b0, const BdfS& S0, int q, int nst, long trial, double tq) {
  {
    HostB a = b0, r = b0;
    BdfS Sa = S0, Sr = S0;
    bdf_rescale(a, Sa);
    ref_rescale(r, Sr);
    same("rescale zn", &a, &r, sizeof a, q, nst, trial);
    same("rescale S", &Sa, &Sr, sizeof Sa, q, nst, trial);
  }
  for (int dq = -1; dq <= 1; dq += 2) {
    HostB a = b0, r = b0;
    BdfS Sa = S0, Sr = S0;
    bdf_adjust_order(a, Sa, dq);
    ref_adjust_order(r, Sr, dq);
    same(dq > 0 ? "adjust+1 zn" : "adjust-1 zn", &a, &r, sizeof a, q, nst, trial);
    same(dq > 0 ? "adjust+1 S" : "adjust-1 S", &Sa, &Sr, sizeof Sa, q, nst, trial);
  }
  {
    const uint64_t a = bits(dky0_lane(b0, S0, tq)), r = bits(ref_dky0(b0, S0, tq));
    same("dky0", &a, &r, 8, q, nst, trial);
  }
  for (int qwait = 0; qwait <= 2; ++qwait) {
    HostB a = b0, r = b0;
    bdf_correct_history(a, S0, S0.q, qwait == 1 && S0.q != QMAX);
    ref_correct_history(r, S0, qwait);
    same("history zn", &a, &r, sizeof a, q, nst, trial);
  }
  {
    BdfS Sa = S0, Sr = S0;
    const uint64_t a = bits(bdf_tau_shift(Sa, Sa.q, Sa.nst, Sa.h)), r = bits(ref_tau_shift(Sr));
    same("tau shift S", &Sa, &Sr, sizeof Sa, q, nst, trial);
    same("tau shift tau2", &a, &r, 8, q, nst, trial);
  }
}

}  // namespace

int main() {
  const int NST[] = {0, 1, 2, 20};
  Gen g(20240607);
  for (int q = 1; q <= QMAX; ++q) {
    for (int nst : NST) {
      // seeded random histories
      for (long trial = 0; trial < 250; ++trial) {
        HostB b;
        BdfS S;
        fill(g, b, S, q, nst);
        run_case(b, S, q, nst, trial, S.tn - S.h * g.unit());
      }
      // every special value in every field the helpers read, one at a time, then a few at once
      for (int k = 0; k < NFIELD; ++k) {
        for (int s = 0; s < NSPECIAL; ++s) {
          HostB b;
          BdfS S;
          fill(g, b, S, q, nst);
          *field(b, S, k) = SPECIAL[s];
          run_case(b, S, q, nst, 1000 + k * NSPECIAL + s, S.tn - 0.5 * S.h);
        }
      }
      for (long trial = 0; trial < 100; ++trial) {
        HostB b;
        BdfS S;
        fill(g, b, S, q, nst);
        for (int m = 0; m < 4; ++m) *field(b, S, (int)(g.r() % NFIELD)) = SPECIAL[g.r() % NSPECIAL];
        const double tq = (trial & 1) ? SPECIAL[g.r() % NSPECIAL] : S.tn;
        run_case(b, S, q, nst, 5000 + trial, tq);
      }
    }
  }
  std::printf("step_control_host: %ld comparisons, %ld mismatches\n", n_checked, n_bad);
  return n_bad == 0 ? 0 : 1;
}
