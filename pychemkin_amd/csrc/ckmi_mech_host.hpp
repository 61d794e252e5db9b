// ckmi_mech_host.hpp -- everything ckmi_mech_create derives from a mechanism descriptor, built on the host.
//
// build_host_mech validates the descriptor and decides what the rate kernels read: the reaction order and
// the type-uniform strips, the annealed lane and unit-slot assignment, the third-body groups, the packed
// LDS image (ckmi_image.hpp) and the workgroup kernel's Jacobian column lists.  It makes no HIP call, so
// the image can be built and checked without a device (tests/mech_image_host.cpp); ckmi_mech_create
// (ckmi.hip) uploads the result.
#pragma once
#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/ckmi.h"
#include "ckmi_image.hpp"

namespace ckmi {
// record the message for ckmi_last_error() and return code: the one way to fail (ckmi.hip)
int set_error(int code, const std::string& msg);

// Slot counts within 0..CKMI_SLOTS and species indices within 0..KK-1 for every reaction, checked
// before any table walk (a descriptor from the C ABI is untrusted); nullptr when valid.
inline const char* check_slots(const ckmi_mech_desc* d) {
  if (!d->nr || !d->np || !d->rsp || !d->psp || !d->rnu || !d->pnu) return "null reaction tables";
  for (int i = 0; i < d->II; ++i) {
    if (d->nr[i] < 0 || d->nr[i] > CKMI_SLOTS || d->np[i] < 0 || d->np[i] > CKMI_SLOTS)
      return "more than 4 species on one side of a reaction (nr / np outside 0..4)";
    for (int u = 0; u < d->nr[i]; ++u)
      if (d->rsp[CKMI_SLOTS * i + u] < 0 || d->rsp[CKMI_SLOTS * i + u] >= d->KK) return "reactant species index out of range";
    for (int u = 0; u < d->np[i]; ++u)
      if (d->psp[CKMI_SLOTS * i + u] < 0 || d->psp[CKMI_SLOTS * i + u] >= d->KK) return "product species index out of range";
  }
  return nullptr;
}
// A reaction the unit-coefficient slots cannot express: a non-integral (or < 1) stoichiometric
// coefficient, a FORD / RORD order that differs from the coefficient, or more than 4 molecules
// on a side.  Evaluated by the extended kernel variants (ckmi_image.hpp eval_gen_img).
inline bool rxn_general(const ckmi_mech_desc* d, int i) {
  int mr = 0, mp = 0;
  for (int u = 0; u < d->nr[i]; ++u) {
    const double nu = d->rnu[CKMI_SLOTS * i + u];
    if (nu != (double)(int)nu || nu < 1.0) return true;
    if (d->ford && d->ford[CKMI_SLOTS * i + u] != nu) return true;
    mr += (int)nu;
  }
  for (int u = 0; u < d->np[i]; ++u) {
    const double nu = d->pnu[CKMI_SLOTS * i + u];
    if (nu != (double)(int)nu || nu < 1.0) return true;
    if (d->rord && d->rord[CKMI_SLOTS * i + u] != nu) return true;
    mp += (int)nu;
  }
  return mr > 4 || mp > 4 || d->nr[i] > 4 || d->np[i] > 4;
}

struct HostMech {
  int KK = 0, II = 0, IIpad = 0, G = 0;
  int npe = 0;  // elements of the corrector's element projection (image element table), 0 = none
  bool has_plog = false;     // PLOG / chemically activated / general reactions: extended kernel variants
  bool has_general = false;  // FORD / RORD / non-integral coefficients (rxn_general)
  double tguard_lo = 0.0, tguard_hi = 1e300;  // runaway guard: min_k T_low,k / 2, 2 max_k T_high,k
  std::vector<int> slot_of;     // [II] original reaction -> device slot
  std::vector<int> orig;        // [IIpad] device slot -> original reaction, -1 for a pad slot
  std::vector<int> rtype_orig;  // [II] CKMI_RXN_* as given
  std::vector<double> lnA_orig, b_orig, E_orig;  // [II] forward Arrhenius (original order) for get / set
  // global-memory species tables (MechDev, ckmi_device.hpp)
  std::vector<double> wt, rwt;  // [KK] W, 1 / W
  std::vector<double> th;       // [17][KK] tlow, tmid, thigh, low a1..a7, high a1..a7 (coefficient-major)
  // the image: scalar fields and offsets (the four device pointers stay null here), its bytes, and the
  // Jacobian column lists MechImage::jcol_ptr / jcol_ent point to once uploaded
  MechImage img{};
  std::vector<char> blob;         // [img.bytes]
  std::vector<int> jcol_ptr;      // [KK + 1]
  std::vector<uint32_t> jcol_ent;  // [max(1, jcol_ptr[KK])]
};

// Validate d and fill h; CKMI_OK, or the code of the first refusal with its text in ckmi_last_error().
// anneal_lanes = false keeps the file order of lanes and unit slots (the CKMI_LANES=0 A/B knob).
int build_host_mech(const ckmi_mech_desc* d, bool anneal_lanes, HostMech& h);
}  // namespace ckmi
