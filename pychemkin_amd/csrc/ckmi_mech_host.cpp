// ckmi_mech_host.cpp -- build_host_mech: the mechanism image and its companions, host code only
// (ckmi_mech_host.hpp).
#include "ckmi_mech_host.hpp"

#include <algorithm>
#include <array>
#include <cmath>
#include <map>
#include <utility>

#include "ckmi_run.hpp"

using namespace ckmi;

namespace {

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
int strip_cost(const std::vector<Rx>& rx, const std::vector<int>& lane_rx, int s0) {
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

// One build: the per-slot tables between the descriptor and the image.  The steps run in the order of
// build_host_mech, each reading what the ones before it left.
struct Builder {
  const ckmi_mech_desc* d;
  HostMech& m;
  std::vector<int> slots;  // device slot -> original reaction (-1 pad)
  std::vector<int> blk;    // (rtype, slot class) block of each reaction: lanes swap within one
  std::vector<std::array<uint8_t, 8>> perm;  // unit-slot order of each reaction (reactant slots 0..3, product 4..7)
  // per device slot ([IIpad]; fp [5][IIpad], rnu / pnu [SLOTS][IIpad])
  std::vector<int> flags, nrp, tb;
  std::vector<std::array<int, 4>> rsp, psp;
  std::vector<double> rnu, pnu, lnA, beta, Ea, lnA0, beta0, Ea0, fp, rlnA, rbeta, rEa;
  // third-body groups (distinct efficiency lists)
  std::vector<int> gptr{0}, gsp;
  std::vector<double> geff;

  int check_records() const;
  void order_slots();
  void assign_lanes();
  int fill_slots();
  int pack_image();
};

// reaction types and the Chebyshev / PLOG records
int Builder::check_records() const {
  for (int i = 0; i < d->II; ++i) {
    if (d->rtype[i] < 0 || d->rtype[i] > CKMI_RXN_LT) return set_error(CKMI_ERR_UNSUPPORTED, "unsupported reaction type");
    if (d->rtype[i] == CKMI_RXN_CHEB) {
      const int p0 = d->plog_ptr ? d->plog_ptr[i] : 0, nrow = d->plog_ptr ? d->plog_ptr[i + 1] - p0 : 0;
      const double* r = d->plog_par ? d->plog_par + 4 * p0 : nullptr;
      const int nt = r && nrow >= 2 ? (int)r[0] : 0, npr = r && nrow >= 2 ? (int)r[1] : 0;
      const bool ok = r && nt >= 1 && nt <= 12 && npr >= 1 && npr <= 12 && nrow == 2 + (nt * npr + 3) / 4 &&
                      r[4] > 0.0 && r[5] > r[4] && r[6] > 0.0 && r[7] > r[6] && !d->has_rev[i];
      if (!ok)
        return set_error(CKMI_ERR_UNSUPPORTED, "Chebyshev record must hold 1..12 x 1..12 coefficients, increasing "
                                               "positive ranges and no REV");
    }
    if (d->rtype[i] == CKMI_RXN_PLOG) {
      const int p0 = d->plog_ptr ? d->plog_ptr[i] : 0, n = d->plog_ptr ? d->plog_ptr[i + 1] - p0 : 0;
      bool ok = d->plog_par && n >= 1 && n <= 64 && !d->has_rev[i];
      for (int j = 0; ok && j + 1 < n; ++j) ok = d->plog_par[4 * (p0 + j)] < d->plog_par[4 * (p0 + j + 1)];
      if (!ok)
        return set_error(CKMI_ERR_UNSUPPORTED, "PLOG table must hold 1..64 points with ascending pressures and no REV");
    }
  }
  return CKMI_OK;
}

// order reactions: elementary, then third-body, then falloff ...; pad to whole strips
void Builder::order_slots() {
  const int II = d->II;
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
  blk.assign(II, -1);
  for (int t : {CKMI_RXN_ELEMENTARY, CKMI_RXN_LT, CKMI_RXN_THIRDBODY, CKMI_RXN_FALLOFF, CKMI_RXN_CHEMACT, CKMI_RXN_PLOG,
                CKMI_RXN_CHEB})
    for (int cls = 0; cls < 3; ++cls)
      for (int i = 0; i < II; ++i)
        if (d->rtype[i] == t && slot_class(i) == cls) {
          ordr.push_back(i);
          blk[i] = 8 * t + cls;
        }
  // pad the elementary block to a 64 multiple when it does not add a strip
  int nelem = 0;
  for (int i = 0; i < II; ++i) nelem += d->rtype[i] == 0;
  const int strips_nopad = (II + WAVE - 1) / WAVE;
  const int elem_pad = (nelem + WAVE - 1) / WAVE * WAVE;
  const int strips_pad = (elem_pad + (II - nelem) + WAVE - 1) / WAVE;
  const bool pad = nelem > 0 && nelem < II && strips_pad == strips_nopad;
  for (int s = 0; s < (int)ordr.size(); ++s) {
    if (pad && s == nelem)
      while ((int)slots.size() < elem_pad) slots.push_back(-1);
    slots.push_back(ordr[s]);
  }
  m.IIpad = std::max(WAVE, (int)((slots.size() + WAVE - 1) / WAVE * WAVE));
  while ((int)slots.size() < m.IIpad) slots.push_back(-1);
}

// slots is reordered in place within (rtype, slot class) blocks; perm receives the unit-slot orders
void Builder::assign_lanes() {
  using lanes::Rx;
  const int II = d->II, n = (int)slots.size();
  std::vector<Rx> rx(II);
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

// the per-slot tables, slot_of / orig and the third-body groups; refuses what a general reaction may not be
int Builder::fill_slots() {
  const int II = d->II, IIpad = m.IIpad;
  std::map<std::vector<std::pair<int, double>>, int> gmap;
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
  m.slot_of.assign(II, -1);
  m.orig.assign(IIpad, -1);
  flags.assign(IIpad, 0), nrp.assign(IIpad, 0), tb.assign(IIpad, -1);
  rsp.assign(IIpad, {0, 0, 0, 0}), psp.assign(IIpad, {0, 0, 0, 0});
  rnu.assign(SLOTS * IIpad, 0.0), pnu.assign(SLOTS * IIpad, 0.0);
  for (auto* v : {&lnA, &beta, &Ea, &lnA0, &beta0, &Ea0, &rlnA, &rbeta, &rEa}) v->assign(IIpad, 0.0);
  fp.assign(5 * IIpad, 1.0);
  for (int s = 0; s < IIpad; ++s) {
    const int i = slots[s];
    m.orig[s] = i;
    if (i < 0) continue;
    m.slot_of[i] = s;
    const bool chemact = d->rtype[i] == CKMI_RXN_CHEMACT;  // device type 2 + info bit 13
    const bool cheb = d->rtype[i] == CKMI_RXN_CHEB;        // device type 3 (rate from the aux stream) + bit 15
    const bool lt = d->rtype[i] == CKMI_RXN_LT;            // device type 0 + bit 15 (B, C in the aux record)
    const int type = chemact ? CKMI_RXN_FALLOFF : (cheb ? CKMI_RXN_PLOG : (lt ? CKMI_RXN_ELEMENTARY : d->rtype[i]));
    flags[s] = type | (d->rev[i] ? 4 : 0) | (d->has_rev[i] ? 8 : 0) | ((d->ftype[i] & 7) << 4) | (chemact ? 0x2000 : 0) |
               ((cheb || lt) ? (int)RX_ALT : 0);
    const int nr = d->nr[i], np = d->np[i];
    if (rxn_general(d, i)) {  // FORD / RORD / non-integral: real coefficients, extended variants
      if (type == CKMI_RXN_PLOG || lt)
        return set_error(CKMI_ERR_UNSUPPORTED,
                         "FORD / RORD or non-integral coefficients on a PLOG, Chebyshev or Landau-Teller reaction");
      for (int u = 0; u < nr; ++u)
        if (!(d->rnu[i * CKMI_SLOTS + u] > 0.0) || (d->ford && d->ford[i * CKMI_SLOTS + u] < 0.0))
          return set_error(CKMI_ERR_UNSUPPORTED, "stoichiometric coefficients must be > 0 and orders >= 0");
      for (int u = 0; u < np; ++u)
        if (!(d->pnu[i * CKMI_SLOTS + u] > 0.0) || (d->rord && d->rord[i * CKMI_SLOTS + u] < 0.0))
          return set_error(CKMI_ERR_UNSUPPORTED, "stoichiometric coefficients must be > 0 and orders >= 0");
      flags[s] |= RX_GEN;
    }
    // (not reachable from a descriptor: check_slots bounds nr / np by CKMI_SLOTS = GEN_SLOTS, and rxn_general
    // holds for more than SLOTS species on a side; kept against a change of either)
    if (nr > GEN_SLOTS || np > GEN_SLOTS || ((nr > SLOTS || np > SLOTS) && !(flags[s] & RX_GEN)))
      return set_error(CKMI_ERR_UNSUPPORTED, "more than 8 species on a reaction side");
    nrp[s] = nr | (np << 8);
    // the per-slot tables hold the first SLOTS species (a general reaction reads its aux stream)
    for (int u = 0; u < nr && u < SLOTS; ++u) {
      rsp[s][u] = d->rsp[i * CKMI_SLOTS + u];
      rnu[u * IIpad + s] = d->rnu[i * CKMI_SLOTS + u];
    }
    for (int u = 0; u < np && u < SLOTS; ++u) {
      psp[s][u] = d->psp[i * CKMI_SLOTS + u];
      pnu[u * IIpad + s] = d->pnu[i * CKMI_SLOTS + u];
    }
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
  m.G = (int)gmap.size();
  return CKMI_OK;
}

// Pack the compact mechanism image (ckmi_image.hpp) from the device-slot tables.
int Builder::pack_image() {
  const int KK = m.KK, IIp = m.IIpad, G = m.G;
  const int KKp = (KK + 1 + WAVE - 1) / WAVE * WAVE;  // room for the dummy species slot
  const int sp_one = KKp - 1;                          // = SP_ONE (63) whenever KK <= 63
  std::vector<uint32_t> urs(IIp, 0), ups(IIp, 0), unu(IIp, 0), uinfo(IIp, 0);
  std::vector<double> aux;
  int naux = 0;
  for (int s = 0; s < IIp; ++s) {
    const int nr = nrp[s] & 0xff, np = nrp[s] >> 8;
    uint32_t a = 0, b = 0, nu = 0;
    const bool gen = (flags[s] & RX_GEN) != 0;  // real coefficients: no unit slots, aux stream
    // unit-coefficient slots: a species with coefficient c occupies c slots
    int ns_r = 0, ns_p = 0;
    int ur[4] = {0, 0, 0, 0}, up[4] = {0, 0, 0, 0};  // unit slots in file order, then in assign_lanes' order
    for (int u = 0; u < nr && !gen; ++u) {
      const int c = (int)rnu[u * IIp + s];
      nu |= (uint32_t)std::min(c, 15) << (4 * u);
      for (int k = 0; k < c; ++k, ++ns_r)
        if (ns_r < 4) ur[ns_r] = rsp[s][u];
    }
    for (int u = 0; u < np && !gen; ++u) {
      const int c = (int)pnu[u * IIp + s];
      nu |= (uint32_t)std::min(c, 15) << (16 + 4 * u);
      for (int k = 0; k < c; ++k, ++ns_p)
        if (ns_p < 4) up[ns_p] = psp[s][u];
    }
    // (not reachable from a descriptor: rxn_general holds for more than 4 molecules on a side, and a general
    // reaction has no unit slots; kept against a change of that rule)
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
    wtp[k] = m.wt[k];
    rwtp[k] = m.rwt[k];
  }
  std::vector<char>& blob = m.blob;
  auto put = [&](const void* p, size_t bytes) -> int {
    const int off = (int)blob.size();
    blob.insert(blob.end(), (const char*)p, (const char*)p + bytes);
    blob.resize(align16((int)blob.size()), 0);
    return off;
  };
  MechImage& I = m.img;
  I.KK = KK;
  I.KKp = KKp;
  I.sp_one = sp_one;
  I.II = m.II;
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
  // the per-slot arrays lie back to back at strides of IIp (IIp is a multiple of 64, so the 16-byte alignment
  // of put() leaves no gap): the reactor kernel's strips address all of them from o_lnA, o_rsp and IIp alone
  // (strip_head, ckmi_reactor.hpp)
  if (!slot_arrays_contiguous(I)) return set_error(CKMI_ERR_ARG, "image layout: per-slot arrays not back to back");
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
    // e-th element that occurs in the mechanism (m.npe of them, <= CKMI_PROJ_MMAX; none otherwise)
    std::vector<uint64_t> el(KKp, 0ull);
    m.npe = 0;
    if (d->ncf && d->MM > 0) {
      std::vector<int> used;
      for (int e = 0; e < d->MM; ++e)
        for (int k = 0; k < KK; ++k)
          if (d->ncf[(size_t)e * KK + k] > 0) {
            used.push_back(e);
            break;
          }
      if ((int)used.size() <= CKMI_PROJ_MMAX) {
        m.npe = (int)used.size();
        for (int j = 0; j < m.npe; ++j)
          for (int k = 0; k < KK; ++k)
            el[k] |= (uint64_t)std::min(255, std::max(0, (int)d->ncf[(size_t)used[j] * KK + k])) << (8 * j);
      }
    }
    const int o_el = put(el.data(), el.size() * 8);
    if (o_el != I.o_e2t + 8 * E2T_N) return set_error(CKMI_ERR_ARG, "image layout: element table not after e2t");
  }
  I.bytes = (int)blob.size();
  {
    // Jacobian column lists of the workgroup kernel (ckmi_big.hip rhs_big): for species j the unit slots
    // naming j, in device-slot order, so that a column block visits only its own slots instead of every
    // slot of every reaction once per block
    std::vector<std::vector<uint32_t>> lists(KK);
    for (int i = 0; i < IIp; ++i) {
      const uint32_t inf = uinfo[i];
      if (inf & RX_GEN) continue;
      const int nr = rx_nr(inf), np = rx_np(inf);
      for (int sl = 0; sl < 8; ++sl) {
        const bool prod = sl >= 4;
        const int u0 = sl & 3;
        if (u0 >= (prod ? np : nr)) continue;
        const int j = sp_of(prod ? ups[i] : urs[i], u0);
        if (j < KK) lists[j].push_back((uint32_t)i | ((uint32_t)sl << 16));
      }
    }
    m.jcol_ptr.assign(KK + 1, 0);
    for (int j = 0; j < KK; ++j) {
      m.jcol_ent.insert(m.jcol_ent.end(), lists[j].begin(), lists[j].end());
      m.jcol_ptr[j + 1] = (int)m.jcol_ent.size();
    }
    if (m.jcol_ent.empty()) m.jcol_ent.push_back(0u);
  }
  return CKMI_OK;
}

}  // namespace

int ckmi::build_host_mech(const ckmi_mech_desc* d, bool anneal_lanes, HostMech& m) {
  const int KK = d->KK, II = d->II;
  if (KK <= 0 || II < 0) return set_error(CKMI_ERR_SIZE, "bad sizes");
  if (KK > KK_IMAGE_MAX) return set_error(CKMI_ERR_UNSUPPORTED, "more than 255 species not supported by this build");
  // slot counts and species indices first: everything below (rxn_general, the slot classes, the
  // image) reads [CKMI_SLOTS i + u] for u < nr[i] / np[i]
  if (const char* bad = check_slots(d)) return set_error(CKMI_ERR_ARG, bad);
  m = HostMech();
  m.KK = KK;
  m.II = II;
  {  // runaway guard range from the NASA-7 fits
    double tlo = 1e300, thi = 0.0;
    for (int k = 0; k < KK; ++k) {
      tlo = std::min(tlo, d->thermo[17 * k + 0]);
      thi = std::max(thi, d->thermo[17 * k + 2]);
    }
    m.tguard_lo = 0.5 * tlo;
    m.tguard_hi = 2.0 * thi;  // margin: legitimately hot runs extrapolate the fits (runaways reach 8-10k K)
  }
  Builder b{d, m};
  if (int rc = b.check_records()) return rc;
  b.order_slots();
  b.perm.assign(II, {0, 1, 2, 3, 0, 1, 2, 3});
  if (anneal_lanes) b.assign_lanes();
  if (int rc = b.fill_slots()) return rc;
  m.rtype_orig.assign(d->rtype, d->rtype + II);
  // PLOG and chemically activated reactions are evaluated by the extended kernel variant
  for (int i = 0; i < II; ++i) {
    const int t = d->rtype[i];
    m.has_plog = m.has_plog || t == CKMI_RXN_PLOG || t == CKMI_RXN_CHEMACT || t == CKMI_RXN_CHEB || t == CKMI_RXN_LT;
    m.has_general = m.has_general || rxn_general(d, i);
  }
  m.has_plog = m.has_plog || m.has_general;
  m.lnA_orig.resize(II);
  m.b_orig.resize(II);
  m.E_orig.resize(II);
  for (int i = 0; i < II; ++i) {
    m.lnA_orig[i] = d->arr[3 * i];
    m.b_orig[i] = d->arr[3 * i + 1];
    m.E_orig[i] = d->arr[3 * i + 2];
  }
  m.wt.assign(d->wt, d->wt + KK);
  m.rwt.resize(KK);
  m.th.resize(17 * KK);
  for (int k = 0; k < KK; ++k) {
    m.rwt[k] = 1.0 / m.wt[k];
    for (int c = 0; c < 17; ++c) m.th[c * KK + k] = d->thermo[17 * k + c];
  }
  return b.pack_image();
}
