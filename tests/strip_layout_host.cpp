// strip_layout_host.cpp -- the layout the reactor kernel's strips rely on (strip_head, ckmi_reactor.hpp), checked
// on images built on the host: a stand-alone program linked with the image builder (ckmi_mech_host.cpp) and the
// native parser (ckmi_parse.cpp), compiled host-only with the host sanitizers and run directly (no GPU).
//
//   strip_layout_host chem thermo [chem thermo ...]
//
// For every input, with the annealed lane assignment and in file order:
//  * the eight per-slot arrays lie back to back: lnA, beta, Ea at strides of 8 IIp bytes from o_lnA, then rsp,
//    psp, nu, info, tb at strides of 4 IIp bytes from o_rsp = o_lnA + 24 IIp, and aux starts where tb ends.  The
//    offsets are compared, and the bytes too: entry i of every array, read at o_lnA + k 8 IIp + 8 i (o_rsp + k 4
//    IIp + 4 i), is what the array's own offset gives;
//  * IIp is a multiple of 64, at least 64, and covers every slot in use;
//  * a padding slot (no reaction) is a valid read that the strips skip: info has nr = np = 0 and no general-
//    reaction bit, and its Arrhenius terms are zero.
// Output: one "layout ..." line per build with KK, II, IIp, the slots in use (1 + the largest slot of a reaction)
// and the padding slots below that count, and a summary line; exit code 1 on any violation.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>

#include "../pychemkin_amd/csrc/ckmi_mech_host.hpp"
#include "../pychemkin_amd/csrc/ckmi_run.hpp"

using namespace ckmi;

namespace {
long g_cases = 0, g_bad = 0;
std::string g_where, g_msg;

void check(bool ok, const char* what, long a = 0, long b = 0) {
  ++g_cases;
  if (ok) return;
  if (++g_bad <= 40) std::printf("VIOLATION %s: %s (%ld, %ld)\n", g_where.c_str(), what, a, b);
}
template <class T>
T at(const HostMech& h, long off) {
  T v;
  std::memcpy(&v, h.blob.data() + off, sizeof(T));
  return v;
}

void check_layout(const HostMech& h) {
  const MechImage& I = h.img;
  const long IIp = I.IIp;
  check(IIp == h.IIpad && IIp >= 64 && IIp % 64 == 0, "IIp a multiple of 64", IIp);
  const int od[3] = {I.o_lnA, I.o_beta, I.o_Ea};
  const int ow[5] = {I.o_rsp, I.o_psp, I.o_nu, I.o_info, I.o_tb};
  for (int k = 0; k < 3; ++k) check(od[k] == I.o_lnA + k * 8 * IIp, "double array at o_lnA + k 8 IIp", k, od[k]);
  check(I.o_rsp == I.o_lnA + 24 * IIp, "o_rsp follows Ea", I.o_rsp);
  for (int k = 0; k < 5; ++k) check(ow[k] == I.o_rsp + k * 4 * IIp, "word array at o_rsp + k 4 IIp", k, ow[k]);
  check(I.o_aux == I.o_rsp + 20 * IIp, "aux follows tb", I.o_aux);
  check(I.o_lnA >= 0 && I.o_lnA % 8 == 0 && I.o_aux <= I.bytes && I.bytes == (int)h.blob.size(), "arrays inside the image");
  if (g_bad) return;
  // the bytes: what the strips read from two bases and the stride is what the view's own offsets give
  for (long i = 0; i < IIp; ++i) {
    for (int k = 0; k < 3; ++k) {
      const uint64_t a = at<uint64_t>(h, I.o_lnA + k * 8 * IIp + 8 * i), b = at<uint64_t>(h, od[k] + 8 * i);
      check(a == b, "double entry by stride", k, i);
    }
    for (int k = 0; k < 5; ++k) {
      const uint32_t a = at<uint32_t>(h, I.o_rsp + k * 4 * IIp + 4 * i), b = at<uint32_t>(h, ow[k] + 4 * i);
      check(a == b, "word entry by stride", k, i);
    }
  }
  int used = 0, pads = 0;
  for (int i = 0; i < h.II; ++i) used = h.slot_of[i] + 1 > used ? h.slot_of[i] + 1 : used;
  check(used <= IIp && IIp - used < 64 + (h.II == 0 ? 1 : 0), "IIp is the slots in use rounded up", used, IIp);
  for (long s = 0; s < IIp; ++s) {
    if (h.orig[s] >= 0) continue;
    pads += s < used;
    const uint32_t inf = at<uint32_t>(h, I.o_info + 4 * s);
    check(rx_nr(inf) == 0 && rx_np(inf) == 0 && !(inf & RX_GEN), "padding slot is skipped", s, inf);
    check(at<double>(h, I.o_lnA + 8 * s) == 0.0 && at<double>(h, I.o_beta + 8 * s) == 0.0 &&
              at<double>(h, I.o_Ea + 8 * s) == 0.0,
          "padding slot has zero Arrhenius terms", s);
  }
  std::printf("layout %s KK %d II %d IIp %ld used %d pads_inside %d\n", g_where.c_str(), h.KK, h.II, IIp, used, pads);
}
}  // namespace

int ckmi::set_error(int code, const std::string& msg) {
  g_msg = msg;
  return code;
}

int main(int argc, char** argv) {
  if (argc < 3 || (argc - 1) % 2) {
    std::fprintf(stderr, "usage: strip_layout_host chem thermo [chem thermo ...]\n");
    return 2;
  }
  int inputs = 0;
  for (int a = 1; a < argc; a += 2, ++inputs) {
    ckmi_parsed* p = nullptr;
    if (ckmi_parse_files(argv[a], argv[a + 1], &p)) {
      std::fprintf(stderr, "%s: %s\n", argv[a], ckmi_parse_last_error());
      return 2;
    }
    ckmi_mech_desc d;
    ckmi_parsed_desc(p, &d);
    if (d.II == 0) {  // the parser's empty tables are null pointers, which the builder refuses: empty, not null
      static const int32_t no_i[1] = {0};
      static const double no_d[1] = {0.0};
      d.nr = d.np = d.rsp = d.psp = no_i, d.rnu = d.pnu = no_d;
    }
    for (int annealed = 1; annealed >= 0; --annealed) {
      g_where = std::string(argv[a]) + (annealed ? " annealed" : " file_order");
      HostMech h;
      const int rc = build_host_mech(&d, annealed != 0, h);
      check(rc == CKMI_OK, g_msg.c_str(), rc);
      if (rc == CKMI_OK) check_layout(h);
    }
    ckmi_parsed_free(p);
  }
  std::printf("strip_layout_host: %d inputs, %ld checks, %ld violations\n", inputs, g_cases, g_bad);
  return g_bad ? 1 : 0;
}
