// mech_image_host.cpp -- the mechanism image of build_host_mech (pychemkin_amd/csrc/ckmi_mech_host.cpp) checked
// against the descriptor it was built from, on the host.  Built and run by tests/test_mech_image_host.py: linked
// with the builder and the native parser, compiled host-only with -fsanitize=address,undefined and run directly
// (no GPU, no Python process).
//
//   mech_image_host [--dump DIR] chem thermo [chem thermo ...]
//
// Every input is parsed (ckmi_parse_files), built with the annealed lane assignment and without, and each image
// is decoded with the image's own helpers (rx_type .. rx_aux, sp_of, nur_of, nup_of) and compared with the
// parsed ckmi_mech_desc: slots, strips, unit slots, rate parameters and flags, aux records, third bodies,
// species tables, the image's tail, its layout, the Jacobian column lists, determinism.  Then every refusal of
// the builder that a descriptor can reach is reached by mutating a parsed one.  Output: one "feature NAME COUNT"
// line per feature met, one "refusal NAME COUNT" line per refusal, and the summary line
//   mech_image_host: C cases, M mismatches
// --dump DIR writes each build's bytes (sizes, MechImage scalars, slot_of, orig, jcol, wt, rwt, th, blob) to
// DIR/<input index>_<0|1 annealed>.bin, for a digest to compare across versions of the builder.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "../pychemkin_amd/csrc/ckmi_mech_host.hpp"
#include "../pychemkin_amd/csrc/ckmi_run.hpp"

using namespace ckmi;

namespace {
int g_code = 0;
std::string g_msg;
long g_cases = 0, g_bad = 0;
std::map<std::string, long> g_feature, g_refusal;
std::string g_where;

void check(bool ok, const char* what, long a = 0, long b = 0) {
  ++g_cases;
  if (ok) return;
  if (++g_bad <= 40) std::printf("MISMATCH %s: %s (%ld, %ld)\n", g_where.c_str(), what, a, b);
}
bool same(double a, double b) { return std::memcmp(&a, &b, 8) == 0; }

template <class T>
const T* at(const HostMech& h, int off) {
  return reinterpret_cast<const T*>(h.blob.data() + off);
}

int device_type(int rtype) {
  return rtype == CKMI_RXN_CHEMACT ? CKMI_RXN_FALLOFF
                                   : (rtype == CKMI_RXN_CHEB ? CKMI_RXN_PLOG : (rtype == CKMI_RXN_LT ? 0 : rtype));
}
// the species of one side expanded by coefficient, in file order
std::vector<int> expand(const ckmi_mech_desc& d, int i, bool prod) {
  std::vector<int> v;
  const int n = prod ? d.np[i] : d.nr[i];
  for (int u = 0; u < n; ++u)
    for (int k = 0; k < (int)(prod ? d.pnu : d.rnu)[CKMI_SLOTS * i + u]; ++k) v.push_back((prod ? d.psp : d.rsp)[CKMI_SLOTS * i + u]);
  return v;
}
// The (reaction type, slot class) block of a reaction, numbered in the order the builder lays the blocks out:
// elementary, Landau-Teller, third body, falloff, chemically activated, PLOG, Chebyshev, and within a type the
// reactions with at most 2 unit slots per side, those with more, the general ones.  Lanes swap within a block only.
int block_rank(const ckmi_mech_desc& d, int i) {
  static const int rank[] = {0, 2, 3, 5, 4, 6, 1};  // by CKMI_RXN_*
  const int cls = rxn_general(&d, i) ? 2 : (expand(d, i, false).size() > 2 || expand(d, i, true).size() > 2 ? 1 : 0);
  return 3 * rank[d.rtype[i]] + cls;
}

void check_image(const ckmi_mech_desc& d, const HostMech& h, bool annealed, bool count_features) {
  const MechImage& I = h.img;
  const int KK = d.KK, II = d.II, IIp = h.IIpad, KKp = (KK + 1 + 63) / 64 * 64;
  // ---- sizes and layout
  check(h.KK == KK && h.II == II && I.KK == KK && I.II == II && I.IIp == IIp && I.G == h.G, "sizes");
  check(IIp % 64 == 0 && IIp >= 64, "IIp a multiple of 64, at least 64", IIp);
  check(I.KKp == KKp && I.sp_one == KKp - 1, "KKp / sp_one", I.KKp, I.sp_one);
  check(I.blob == nullptr && I.slot_of == nullptr && I.jcol_ptr == nullptr && I.jcol_ent == nullptr, "device pointers null");
  check(I.bytes == (int)h.blob.size() && I.bytes % 16 == 0, "bytes == blob.size()", I.bytes, (long)h.blob.size());
  if (I.bytes != (int)h.blob.size() || I.IIp != IIp || I.KKp != KKp) return;
  const int ng = I.G >= 0 && I.o_gptr + 4 * (I.G + 1) <= I.bytes ? at<int>(h, I.o_gptr)[I.G] : -1;
  check(ng >= 0, "gptr[G]", ng);
  if (ng < 0) return;
  const bool dense = I.o_e2t - I.o_geffd > 16;  // MechView::mgt()
  {
    const int off[] = {I.o_th, I.o_wt, I.o_rwt, I.o_lnA, I.o_beta, I.o_Ea, I.o_rsp, I.o_psp, I.o_nu, I.o_info, I.o_tb,
                       I.o_aux, I.o_gptr, I.o_gsp, I.o_geff, I.o_geffd, I.o_e2t, I.o_e2t + 8 * E2T_N, I.bytes};
    const int size[] = {15 * KKp * 8, KKp * 8, KKp * 8, IIp * 8, IIp * 8, IIp * 8, IIp * 4, IIp * 4, IIp * 4, IIp * 4,
                        IIp * 4, I.naux * AUXW * 8, (I.G + 1) * 4, std::max(ng, 1) * 4, std::max(ng, 1) * 8,
                        dense ? 64 * 17 * 8 : 16, 8 * E2T_N, KKp * 8};
    check(off[0] == 0, "image starts at th", off[0]);
    for (int k = 0; k < 18; ++k) {
      check(off[k] % 16 == 0 && off[k + 1] > off[k], "offsets 16-aligned and increasing", k, off[k]);
      check(off[k + 1] == off[k] + ((size[k] + 15) & ~15), "segment size", k, off[k + 1] - off[k]);
    }
    if (g_bad) return;  // the decoders below trust the layout
    const size_t lds_with = (size_t)I.o_geffd + 64 * 17 * 8 + 8 * E2T_N + 8 * (size_t)KKp + jscratch_bytes<64>() +
                            12 * (size_t)slice_bytes(I.G);
    check(dense == (KK <= SP_ONE && I.G <= 16 && lds_with <= 160 * 1024), "dense geffd where the wave kernel's LDS holds it");
  }
  const double *lnA = at<double>(h, I.o_lnA), *beta = at<double>(h, I.o_beta), *Ea = at<double>(h, I.o_Ea);
  const uint32_t *rsp = at<uint32_t>(h, I.o_rsp), *psp = at<uint32_t>(h, I.o_psp), *nu = at<uint32_t>(h, I.o_nu);
  const uint32_t* info = at<uint32_t>(h, I.o_info);
  const int* tb = at<int>(h, I.o_tb);
  const double* aux = at<double>(h, I.o_aux);
  const int *gptr = at<int>(h, I.o_gptr), *gsp = at<int>(h, I.o_gsp);
  const double *geff = at<double>(h, I.o_geff), *geffd = at<double>(h, I.o_geffd);
  const uint32_t one = (uint32_t)I.sp_one, all_one = one | one << 8 | one << 16 | one << 24;
  // ---- slots
  check((int)h.slot_of.size() == II && (int)h.orig.size() == IIp, "slot_of / orig sizes");
  int nonpad = 0, last_real = -1;
  for (int s = 0; s < IIp; ++s) {
    const int i = h.orig[s];
    if (i >= 0) {
      ++nonpad, last_real = s;
      check(i < II && h.slot_of[i] == s, "slot_of[orig[s]] == s", s, i);
    } else {
      check(rx_nr(info[s]) == 0 && rx_np(info[s]) == 0 && rsp[s] == all_one && psp[s] == all_one && tb[s] == -1 &&
                same(lnA[s], 0.0),
            "pad slot empty", s);
    }
  }
  check(nonpad == II, "as many non-pad slots as reactions", nonpad, II);
  for (int i = 0; i < II; ++i) check(h.slot_of[i] >= 0 && h.slot_of[i] < IIp && h.orig[h.slot_of[i]] == i, "orig[slot_of[i]] == i", i);
  bool pad_taken = false;
  for (int s = 0; s < last_real; ++s) pad_taken = pad_taken || h.orig[s] < 0;
  // ---- strips.  The blocks follow each other in block_rank order, so the device type never decreases along
  // the slots, and only the elementary block is padded to whole strips, where that adds no strip: a strip past it
  // may hold the end of one type and the start of the next (GRI-Mech 3.0: third-body slots up to 331, falloff
  // from 332; the kernels take the type per lane).  So: block order in both modes, file order within a block
  // without annealing, the padding rule, and no strip that mixes elementary reactions with others once padded.
  {
    int prev = -1, nelem = 0, mixed = 0;
    for (int i = 0; i < II; ++i) nelem += d.rtype[i] == CKMI_RXN_ELEMENTARY;
    for (int s = 0; s < IIp; ++s) {
      const int i = h.orig[s];
      if (i < 0) continue;
      if (prev >= 0) {
        check(block_rank(d, prev) <= block_rank(d, i), "blocks in order", prev, i);
        check(rx_type(info[h.slot_of[prev]]) <= rx_type(info[s]), "device type never decreases", s);
        if (!annealed && block_rank(d, prev) == block_rank(d, i)) check(prev < i, "file order within a block", prev, i);
      }
      prev = i;
    }
    const int elem_pad = (nelem + 63) / 64 * 64;
    const bool want_pad = nelem > 0 && nelem < II && (elem_pad + (II - nelem) + 63) / 64 == (II + 63) / 64;
    check(pad_taken == (want_pad && elem_pad > nelem), "elementary block padded exactly where that adds no strip");
    for (int s = 0; s < last_real; ++s)
      if (h.orig[s] < 0) check(want_pad && s >= nelem && s < elem_pad, "interior pad slots close the elementary block", s);
    for (int s0 = 0; s0 < IIp; s0 += 64) {
      int ne = 0, no = 0, tmin = 3, tmax = 0;
      for (int s = s0; s < s0 + 64; ++s) {
        if (h.orig[s] < 0) continue;
        (d.rtype[h.orig[s]] == CKMI_RXN_ELEMENTARY ? ne : no) += 1;
        tmin = std::min(tmin, rx_type(info[s])), tmax = std::max(tmax, rx_type(info[s]));
      }
      if (want_pad) check(ne == 0 || no == 0, "padded: no strip mixes elementary reactions with others", s0);
      mixed += tmax > tmin;
    }
    if (count_features) g_feature["strips_of_two_device_types"] += mixed;
  }
  // ---- per reaction
  std::vector<std::pair<int, int>> recs;  // aux records [first, end) of each reaction that has some
  std::map<std::string, long> feat;
  for (int i = 0; i < II; ++i) {
    const int s = h.slot_of[i];
    const uint32_t inf = info[s];
    const int rt = d.rtype[i], type = device_type(rt);
    const bool gen = rxn_general(&d, i), cheb = rt == CKMI_RXN_CHEB, lt = rt == CKMI_RXN_LT;
    g_where += " rxn " + std::to_string(i);
    check(rx_type(inf) == type, "device type", rx_type(inf), type);
    check(rx_rev(inf) == (d.rev[i] != 0), "rev bit");
    check(rx_hasrev(inf) == (d.has_rev[i] != 0), "has_rev bit");
    check(rx_ftype(inf) == (d.ftype[i] & 7), "ftype", rx_ftype(inf), d.ftype[i]);
    check(((inf & 0x2000u) != 0) == (rt == CKMI_RXN_CHEMACT), "chemically-activated bit");
    check(((inf & RX_ALT) != 0) == (cheb || lt), "RX_ALT");
    check(((inf & RX_GEN) != 0) == gen, "RX_GEN");
    check(h.rtype_orig[i] == rt && same(h.lnA_orig[i], d.arr[3 * i]) && same(h.b_orig[i], d.arr[3 * i + 1]) &&
              same(h.E_orig[i], d.arr[3 * i + 2]),
          "original type and Arrhenius copies");
    // rate parameters
    const bool tab = type == CKMI_RXN_PLOG;
    check(same(lnA[s], tab ? 0.0 : d.arr[3 * i]) && same(beta[s], tab ? 0.0 : d.arr[3 * i + 1]) &&
              same(Ea[s], tab ? 0.0 : d.arr[3 * i + 2]),
          "lnA / beta / Ea");
    // unit slots
    if (gen) {
      check(rx_nr(inf) == 0 && rx_np(inf) == 0 && rsp[s] == all_one && psp[s] == all_one && nu[s] == 0, "general: no unit slots");
    } else {
      for (int side = 0; side < 2; ++side) {
        std::vector<int> want = expand(d, i, side == 1), got;
        const int ns = side ? rx_np(inf) : rx_nr(inf);
        const uint32_t w = side ? psp[s] : rsp[s];
        check(ns == (int)want.size(), "unit slot count", ns, (long)want.size());
        for (int u = 0; u < 4; ++u) {
          if (u < ns) got.push_back(sp_of(w, u));
          else check(sp_of(w, u) == I.sp_one, "unused unit slot holds sp_one", u, sp_of(w, u));
        }
        if (!annealed) check(got == want, "unit slots in file order");
        std::sort(want.begin(), want.end()), std::sort(got.begin(), got.end());
        check(got == want, "unit slot species");
        const int n = side ? d.np[i] : d.nr[i];
        for (int u = 0; u < 4; ++u) {
          const int c = u < n ? (int)(side ? d.pnu : d.rnu)[CKMI_SLOTS * i + u] : 0;
          check((side ? nup_of(nu[s], u) : nur_of(nu[s], u)) == c, "nu nibble", u, c);
          if (c == 2) ++feat["coefficient_2"];
        }
      }
    }
    // aux
    const int a0 = rx_aux(inf);
    int nrec = 0;
    if (cheb) {
      const double* r = d.plog_par + 4 * d.plog_ptr[i];
      const int nt = (int)r[0], npr = (int)r[1];
      nrec = (6 + nt * npr + AUXW - 1) / AUXW;
      if (a0 + nrec <= I.naux) {
        const double* p = aux + AUXW * a0;
        check(same(p[0], nt) && same(p[1], npr) && same(p[2], 1.0 / r[4]) && same(p[3], 1.0 / r[5]) &&
                  same(p[4], std::log10(r[6] * 1.01325e6)) && same(p[5], std::log10(r[7] * 1.01325e6)),
              "Chebyshev header (ranges as 1/T and log10 of dyn/cm2)");
        for (int k = 0; k < nrec * AUXW - 6; ++k) check(same(p[6 + k], k < nt * npr ? r[8 + k] : 0.0), "Chebyshev coefficient", k);
      }
      ++feat["chebyshev"];
    } else if (rt == CKMI_RXN_PLOG) {
      const int p0 = d.plog_ptr[i], n = d.plog_ptr[i + 1] - p0;
      nrec = (1 + 4 * n + AUXW - 1) / AUXW;
      if (a0 + nrec <= I.naux) {
        const double* p = aux + AUXW * a0;
        check(same(p[0], n), "PLOG point count");
        for (int k = 0; k < nrec * AUXW - 1; ++k) check(same(p[1 + k], k < 4 * n ? d.plog_par[4 * p0 + k] : 0.0), "PLOG stream", k);
      }
      ++feat["plog"];
    } else if (type == 2 || d.has_rev[i] || gen || lt) {
      nrec = 1 + (gen ? GEN_RECORDS : 0);
      if (a0 + nrec <= I.naux) {
        const double* p = aux + AUXW * a0;
        const int ft = d.ftype[i] & 7;
        double want[AUXW] = {d.low[3 * i], d.low[3 * i + 1], d.low[3 * i + 2], d.fpar[5 * i], d.fpar[5 * i + 1],
                             d.fpar[5 * i + 2], d.fpar[5 * i + 3], d.fpar[5 * i + 4], d.revp[3 * i], d.revp[3 * i + 1],
                             d.revp[3 * i + 2], 0.0, 0.0};
        if (ft == CKMI_FALL_TROE3 || ft == CKMI_FALL_TROE4) want[4] = 1.0 / want[4], want[5] = 1.0 / want[5];
        if (ft == CKMI_FALL_SRI) want[5] = 1.0 / want[5];
        for (int k = 0; k < AUXW; ++k) check(same(p[k], want[k]), "low / falloff / REV record", k);
        if (gen) {
          const double* g = p + AUXW;
          std::vector<double> w(GEN_RECORDS * AUXW, 0.0);
          w[0] = d.nr[i], w[1] = d.np[i];
          for (int u = 0; u < d.nr[i]; ++u) {
            w[2 + 3 * u] = d.rsp[CKMI_SLOTS * i + u], w[3 + 3 * u] = d.rnu[CKMI_SLOTS * i + u];
            w[4 + 3 * u] = d.ford ? d.ford[CKMI_SLOTS * i + u] : d.rnu[CKMI_SLOTS * i + u];
          }
          for (int u = 0; u < d.np[i]; ++u) {
            w[GEN_P + 3 * u] = d.psp[CKMI_SLOTS * i + u], w[GEN_P + 1 + 3 * u] = d.pnu[CKMI_SLOTS * i + u];
            w[GEN_P + 2 + 3 * u] = d.rord ? d.rord[CKMI_SLOTS * i + u] : d.pnu[CKMI_SLOTS * i + u];
          }
          for (int k = 0; k < GEN_RECORDS * AUXW; ++k) check(same(g[k], w[k]), "general-reaction record", k);
        }
      }
    }
    if (nrec) {
      check(a0 + nrec <= I.naux, "aux records within naux", a0 + nrec, I.naux);
      recs.push_back({a0, a0 + nrec});
    }
    if (type == 2 && ((d.ftype[i] & 7) == CKMI_FALL_TROE3 || (d.ftype[i] & 7) == CKMI_FALL_TROE4)) ++feat["troe"];
    if (type == 2 && (d.ftype[i] & 7) == CKMI_FALL_SRI) ++feat["sri"];
    if (rt == CKMI_RXN_CHEMACT) ++feat["chemically_activated"];
    if (d.has_rev[i]) ++feat["explicit_rev"];
    if (lt) ++feat["landau_teller"];
    if (gen) ++feat["general"];
    // third body
    if (type == 1 || type == 2) {
      if (d.tbsp[i] >= 0) {
        check(tb[s] == -(d.tbsp[i] + 2), "single collider", tb[s], d.tbsp[i]);
        ++feat["collider_third_body"];
      } else {
        check(tb[s] >= 0 && tb[s] < I.G, "third-body group index", tb[s], I.G);
        if (tb[s] >= 0 && tb[s] < I.G) {
          const int g = tb[s];
          std::vector<std::pair<int, double>> want, got;
          for (int p = d.eff_ptr[i]; p < d.eff_ptr[i + 1]; ++p)
            if (d.eff_val[p] != 1.0) want.push_back({d.eff_sp[p], d.eff_val[p] - 1.0});
          std::sort(want.begin(), want.end());
          for (int p = gptr[g]; p < gptr[g + 1]; ++p) got.push_back({gsp[p], geff[p]});
          check(got == want, "third-body group list", g);
        }
        ++feat["group_third_body"];
      }
    } else {
      check(tb[s] == -1, "no third body", tb[s]);
    }
    g_where.resize(g_where.rfind(" rxn "));
  }
  std::sort(recs.begin(), recs.end());
  for (size_t k = 0; k + 1 < recs.size(); ++k) check(recs[k].second <= recs[k + 1].first, "aux records do not overlap", recs[k].second, recs[k + 1].first);
  if (recs.empty()) {
    check(I.naux == 1, "one empty aux record", I.naux);
    for (int k = 0; k < AUXW; ++k) check(same(aux[k], 0.0), "empty aux record", k);
  } else {
    check(recs.front().first == 0 && recs.back().second == I.naux, "aux records fill naux", recs.back().second, I.naux);
  }
  // ---- dense third-body table
  check(gptr[0] == 0, "gptr[0]");
  if (dense) {
    std::vector<double> want(64 * 17, 0.0);
    for (int g = 0; g < I.G; ++g)
      for (int p = gptr[g]; p < gptr[g + 1]; ++p) want[gsp[p] * 17 + g] = geff[p];
    for (int k = 0; k < 64 * 17; ++k) check(same(geffd[k], want[k]), "geffd", k);
  } else {
    check(same(geffd[0], 0.0) && same(geffd[1], 0.0), "geffd stub");
  }
  // ---- species tables
  const double *th = at<double>(h, I.o_th), *wt = at<double>(h, I.o_wt), *rwt = at<double>(h, I.o_rwt);
  check((int)h.wt.size() == KK && (int)h.rwt.size() == KK && (int)h.th.size() == 17 * KK, "species table sizes");
  for (int k = 0; k < KKp; ++k) {
    const bool in = k < KK;
    if (in) {
      check(same(h.wt[k], d.wt[k]) && same(h.rwt[k], 1.0 / d.wt[k]), "wt / rwt", k);
      for (int c = 0; c < 17; ++c) check(same(h.th[c * KK + k], d.thermo[17 * k + c]), "th", k, c);
    }
    check(same(wt[k], in ? d.wt[k] : 0.0) && same(rwt[k], in ? 1.0 / d.wt[k] : 0.0), "image wt / rwt", k);
    check(same(th[k], in ? d.thermo[17 * k + 1] : 0.0), "image tmid", k);
    for (int c = 0; c < 14; ++c) check(same(th[(1 + c) * KKp + k], in ? d.thermo[17 * k + 3 + c] : 0.0), "image NASA-7", k, c);
  }
  {
    double tlo = 1e300, thi = 0.0;
    for (int k = 0; k < KK; ++k) tlo = std::min(tlo, d.thermo[17 * k]), thi = std::max(thi, d.thermo[17 * k + 2]);
    check(same(h.tguard_lo, 0.5 * tlo) && same(h.tguard_hi, 2.0 * thi), "guard temperatures");
  }
  // ---- tail: e2t, then the element table
  const double* e2t = at<double>(h, I.o_e2t);
  for (int j = 0; j < E2T_N; ++j) check(same(e2t[j], (double)std::exp2((long double)j / (long double)E2T_N)), "e2t", j);
  {
    const uint64_t* el = at<uint64_t>(h, I.o_e2t + 8 * E2T_N);
    std::vector<int> used;
    for (int e = 0; d.ncf && e < d.MM; ++e)
      for (int k = 0; k < KK; ++k)
        if (d.ncf[(size_t)e * KK + k] > 0) {
          used.push_back(e);
          break;
        }
    const int npe = (int)used.size() <= CKMI_PROJ_MMAX ? (int)used.size() : 0;
    check(h.npe == npe, "npe", h.npe, npe);
    for (int k = 0; k < KKp; ++k) {
      uint64_t want = 0;
      for (int j = 0; j < npe && k < KK; ++j) want |= (uint64_t)std::min(255, std::max(0, (int)d.ncf[(size_t)used[j] * KK + k])) << (8 * j);
      check(el[k] == want, "element table", k);
    }
  }
  // ---- flags of the whole mechanism
  {
    bool ext = false, gen = false;
    for (int i = 0; i < II; ++i) ext = ext || d.rtype[i] >= CKMI_RXN_PLOG, gen = gen || rxn_general(&d, i);
    check(h.has_general == gen && h.has_plog == (ext || gen), "has_plog / has_general");
  }
  // ---- Jacobian columns
  check((int)h.jcol_ptr.size() == KK + 1 && h.jcol_ptr[0] == 0, "jcol_ptr size");
  {
    std::vector<std::vector<uint32_t>> want(KK);
    for (int s = 0; s < IIp; ++s) {
      if (info[s] & RX_GEN) continue;
      for (int sl = 0; sl < 8; ++sl) {
        const int u = sl & 3;
        if (u >= (sl >= 4 ? rx_np(info[s]) : rx_nr(info[s]))) continue;
        const int j = sp_of(sl >= 4 ? psp[s] : rsp[s], u);
        if (j < KK) want[j].push_back((uint32_t)s | (uint32_t)sl << 16);
      }
    }
    size_t total = 0;
    for (int j = 0; j < KK; ++j) {
      const int p0 = h.jcol_ptr[j], p1 = h.jcol_ptr[j + 1];
      const bool in = p0 >= 0 && p1 >= p0 && (size_t)p1 <= h.jcol_ent.size();
      check(in && std::vector<uint32_t>(h.jcol_ent.begin() + p0, h.jcol_ent.begin() + p1) == want[j], "jcol list", j);
      total += want[j].size();
    }
    check(h.jcol_ptr[KK] == (int)total && h.jcol_ent.size() == std::max<size_t>(total, 1), "jcol_ent size");
  }
  if (!count_features) return;
  for (auto& kv : feat) g_feature[kv.first] += kv.second;
  ++g_feature[pad_taken ? "pad_taken" : "pad_not_taken"];
  ++g_feature[dense ? "geffd_dense" : "geffd_stub"];
  if (h.npe > 0) ++g_feature["npe"];
  if (II == 0) ++g_feature["no_reactions"];
}

// ---------------------------------------------------------------- refusals
// a descriptor whose tables can be changed: copies of the parsed one's
struct Desc {
  ckmi_mech_desc d;
  std::vector<int32_t> rtype, nr, np, rsp, psp, has_rev;
  std::vector<double> rnu, pnu, plog_par, ford, rord;
  explicit Desc(const ckmi_mech_desc& s) : d(s) {
    const size_t II = s.II, npl = s.plog_ptr ? s.plog_ptr[II] : 0;
    rtype.assign(s.rtype, s.rtype + II), nr.assign(s.nr, s.nr + II), np.assign(s.np, s.np + II);
    has_rev.assign(s.has_rev, s.has_rev + II);
    rsp.assign(s.rsp, s.rsp + CKMI_SLOTS * II), psp.assign(s.psp, s.psp + CKMI_SLOTS * II);
    rnu.assign(s.rnu, s.rnu + CKMI_SLOTS * II), pnu.assign(s.pnu, s.pnu + CKMI_SLOTS * II);
    ford.assign(s.ford, s.ford + CKMI_SLOTS * II), rord.assign(s.rord, s.rord + CKMI_SLOTS * II);
    plog_par.assign(s.plog_par, s.plog_par + 4 * npl);
    d.rtype = rtype.data(), d.nr = nr.data(), d.np = np.data(), d.has_rev = has_rev.data();
    d.rsp = rsp.data(), d.psp = psp.data(), d.rnu = rnu.data(), d.pnu = pnu.data();
    d.ford = ford.data(), d.rord = rord.data(), d.plog_par = plog_par.data();
  }
};

void refused(const char* name, const Desc& m, int code, const char* text) {
  HostMech h;
  g_code = 0, g_msg.clear();
  const int rc = build_host_mech(&m.d, false, h);  // (a refusal does not depend on the lane assignment)
  g_where = std::string("refusal ") + name;
  check(rc == code && g_code == code, "code", rc, code);
  check(g_msg == text, g_msg.c_str());
  ++g_refusal[name];
}

constexpr const char* T_GEN_TABLE = "FORD / RORD or non-integral coefficients on a PLOG, Chebyshev or Landau-Teller reaction";
constexpr const char* T_GEN_NU = "stoichiometric coefficients must be > 0 and orders >= 0";
constexpr const char* T_CHEB = "Chebyshev record must hold 1..12 x 1..12 coefficients, increasing positive ranges and no REV";
constexpr const char* T_PLOG = "PLOG table must hold 1..64 points with ascending pressures and no REV";

// Not reached here, because no descriptor reaches them (comments in ckmi_mech_host.cpp): "more than 8 species on
// a reaction side", "more than 4 molecules (sum of coefficients) on a reaction side", "image layout: element
// table not after e2t".
void check_refusals(const ckmi_mech_desc& d) {
  const int II = d.II;
  const auto first = [&](int rtype) {
    for (int i = 0; i < II; ++i)
      if (d.rtype[i] == rtype && d.nr[i] > 0 && d.np[i] > 0) return i;
    return -1;
  };
  {
    Desc m(d);
    m.d.KK = 0;
    refused("bad_sizes_KK", m, CKMI_ERR_SIZE, "bad sizes");
    m.d.KK = d.KK, m.d.II = -1;
    refused("bad_sizes_II", m, CKMI_ERR_SIZE, "bad sizes");
    m.d.II = II, m.d.KK = KK_IMAGE_MAX + 1;
    refused("too_many_species", m, CKMI_ERR_UNSUPPORTED, "more than 255 species not supported by this build");
    m.d.KK = d.KK, m.d.pnu = nullptr;
    refused("null_tables", m, CKMI_ERR_ARG, "null reaction tables");
  }
  const int e = first(CKMI_RXN_ELEMENTARY);
  if (e >= 0) {
    {
      Desc m(d);
      m.nr[e] = CKMI_SLOTS + 1;
      refused("slot_count", m, CKMI_ERR_ARG, "more than 4 species on one side of a reaction (nr / np outside 0..4)");
      m.nr[e] = d.nr[e], m.np[e] = -1;
      refused("slot_count", m, CKMI_ERR_ARG, "more than 4 species on one side of a reaction (nr / np outside 0..4)");
    }
    {
      Desc m(d);
      m.rsp[CKMI_SLOTS * e] = d.KK;
      refused("reactant_index", m, CKMI_ERR_ARG, "reactant species index out of range");
      m.rsp[CKMI_SLOTS * e] = d.rsp[CKMI_SLOTS * e], m.psp[CKMI_SLOTS * e] = -1;
      refused("product_index", m, CKMI_ERR_ARG, "product species index out of range");
    }
    {
      Desc m(d);
      m.rtype[e] = CKMI_RXN_LT + 1;
      refused("reaction_type", m, CKMI_ERR_UNSUPPORTED, "unsupported reaction type");
      m.rtype[e] = -1;
      refused("reaction_type", m, CKMI_ERR_UNSUPPORTED, "unsupported reaction type");
    }
    {
      Desc m(d);
      m.rnu[CKMI_SLOTS * e] = -0.5;
      refused("general_reactant_nu", m, CKMI_ERR_UNSUPPORTED, T_GEN_NU);
      m.rnu[CKMI_SLOTS * e] = 1.5, m.ford[CKMI_SLOTS * e] = -1.0;
      refused("general_forward_order", m, CKMI_ERR_UNSUPPORTED, T_GEN_NU);
    }
    {
      Desc m(d);
      m.pnu[CKMI_SLOTS * e] = 0.0;
      refused("general_product_nu", m, CKMI_ERR_UNSUPPORTED, T_GEN_NU);
      m.pnu[CKMI_SLOTS * e] = 1.5, m.rord[CKMI_SLOTS * e] = -1.0;
      refused("general_reverse_order", m, CKMI_ERR_UNSUPPORTED, T_GEN_NU);
    }
  }
  const int c = first(CKMI_RXN_CHEB);
  if (c >= 0) {
    const int r = 4 * d.plog_ptr[c];
    for (int k = 0; k < 6; ++k) {
      Desc m(d);
      if (k == 0) m.plog_par[r + 0] = 13.0;           // NT
      if (k == 1) m.plog_par[r + 1] = 0.0;            // NP
      if (k == 2) m.plog_par[r + 4] = 0.0;            // Tmin
      if (k == 3) m.plog_par[r + 7] = d.plog_par[r + 6];  // Pmax = Pmin
      if (k == 4) m.has_rev[c] = 1;
      if (k == 5) m.plog_par[r + 5] = d.plog_par[r + 4];  // Tmax = Tmin
      refused("chebyshev_record", m, CKMI_ERR_UNSUPPORTED, T_CHEB);
    }
    Desc m(d);
    m.rnu[CKMI_SLOTS * c] = 1.5;
    refused("general_chebyshev", m, CKMI_ERR_UNSUPPORTED, T_GEN_TABLE);
  }
  const int p = first(CKMI_RXN_PLOG);
  if (p >= 0) {
    const int p0 = d.plog_ptr[p], n = d.plog_ptr[p + 1] - p0;
    for (int k = 0; k < 2; ++k) {
      if (k == 0 && n < 2) continue;
      Desc m(d);
      if (k == 0) m.plog_par[4 * (p0 + 1)] = d.plog_par[4 * p0];  // pressures not ascending
      if (k == 1) m.has_rev[p] = 1;
      refused("plog_table", m, CKMI_ERR_UNSUPPORTED, T_PLOG);
    }
    Desc m(d);
    m.pnu[CKMI_SLOTS * p] = 0.5;
    refused("general_plog", m, CKMI_ERR_UNSUPPORTED, T_GEN_TABLE);
  }
  const int l = first(CKMI_RXN_LT);
  if (l >= 0) {
    Desc m(d);
    m.ford[CKMI_SLOTS * l] = 0.5;
    refused("general_landau_teller", m, CKMI_ERR_UNSUPPORTED, T_GEN_TABLE);
  }
}

void put(FILE* f, const void* p, size_t bytes) { std::fwrite(p, 1, bytes, f); }
template <class T>
void put(FILE* f, const std::vector<T>& v) {
  put(f, v.data(), v.size() * sizeof(T));
}
bool dump(const HostMech& h, const std::string& path) {
  FILE* f = std::fopen(path.c_str(), "wb");
  if (!f) return false;
  const MechImage& I = h.img;
  const int head[] = {h.KK, h.II, h.IIpad, h.G, h.npe, h.has_plog, h.has_general, I.bytes, I.KK, I.KKp, I.II, I.IIp,
                      I.G, I.naux, I.sp_one, I.o_th, I.o_wt, I.o_rwt, I.o_lnA, I.o_beta, I.o_Ea, I.o_rsp, I.o_psp,
                      I.o_nu, I.o_info, I.o_tb, I.o_aux, I.o_gptr, I.o_gsp, I.o_geff, I.o_geffd, I.o_e2t};
  put(f, head, sizeof(head));
  put(f, &h.tguard_lo, 8), put(f, &h.tguard_hi, 8);
  put(f, h.slot_of), put(f, h.orig), put(f, h.jcol_ptr), put(f, h.jcol_ent);
  put(f, h.wt), put(f, h.rwt), put(f, h.th), put(f, h.blob);
  return std::fclose(f) == 0;
}
}  // namespace

int ckmi::set_error(int code, const std::string& msg) {
  g_code = code, g_msg = msg;
  return code;
}

int main(int argc, char** argv) {
  std::string dump_dir;
  int a = 1;
  if (argc > 2 && std::string(argv[1]) == "--dump") dump_dir = argv[2], a = 3;
  if (a >= argc || (argc - a) % 2) {
    std::fprintf(stderr, "usage: mech_image_host [--dump DIR] chem thermo [chem thermo ...]\n");
    return 2;
  }
  for (int n = 0; a < argc; a += 2, ++n) {
    ckmi_parsed* p = nullptr;
    if (ckmi_parse_files(argv[a], argv[a + 1], &p)) {
      std::fprintf(stderr, "%s: %s\n", argv[a], ckmi_parse_last_error());
      return 2;
    }
    ckmi_mech_desc d;
    ckmi_parsed_desc(p, &d);
    if (d.II == 0) {  // the parser's empty tables are null pointers, which check_slots refuses: empty, not null
      static const int32_t no_i[1] = {0};
      static const double no_d[1] = {0.0};
      d.nr = d.np = d.rsp = d.psp = no_i, d.rnu = d.pnu = no_d;
    }
    for (int annealed = 1; annealed >= 0; --annealed) {
      g_where = std::string(argv[a]) + (annealed ? " annealed" : " file order");
      HostMech h, again;
      const int rc = build_host_mech(&d, annealed != 0, h);
      check(rc == CKMI_OK, g_msg.c_str(), rc);
      if (rc) continue;
      check_image(d, h, annealed != 0, annealed != 0);
      check(build_host_mech(&d, annealed != 0, again) == CKMI_OK && again.blob == h.blob && again.slot_of == h.slot_of &&
                again.orig == h.orig && again.jcol_ptr == h.jcol_ptr && again.jcol_ent == h.jcol_ent &&
                std::memcmp(&again.img, &h.img, sizeof(MechImage)) == 0,
            "two builds give the same bytes");
      if (!dump_dir.empty() && !dump(h, dump_dir + "/" + std::to_string(n) + "_" + std::to_string(annealed) + ".bin")) {
        std::fprintf(stderr, "cannot write to %s\n", dump_dir.c_str());
        return 2;
      }
      std::printf("image %s KK %d II %d IIp %d G %d naux %d bytes %d\n", g_where.c_str(), h.KK, h.II, h.IIpad, h.G,
                  h.img.naux, h.img.bytes);
    }
    check_refusals(d);
    ckmi_parsed_free(p);
  }
  for (auto& kv : g_feature) std::printf("feature %s %ld\n", kv.first.c_str(), kv.second);
  for (auto& kv : g_refusal) std::printf("refusal %s %ld\n", kv.first.c_str(), kv.second);
  std::printf("mech_image_host: %ld cases, %ld mismatches\n", g_cases, g_bad);
  return g_bad ? 1 : 0;
}
