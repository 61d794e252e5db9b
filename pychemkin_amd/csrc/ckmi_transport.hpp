// ckmi_transport.hpp -- the device tables behind a ckmi_transport handle, shared by the viscosity /
// conductivity kernels (ckmi_transport.hip) and the diffusion kernels (ckmi_diffusion.hip).
#pragma once

#include <vector>

namespace ckmi_tran {
constexpr double P_ATM = 1.01325e6;  // dyn/cm2: the pressure of the binary diffusion fits
}

struct ckmi_transport {
  int device = 0;
  int KK = 0;
  double* fits = nullptr;  // device [KK][4]
  double* A = nullptr;     // device [KK][KK]
  double* B = nullptr;     // device [KK][KK]
  double* cfits = nullptr; // device [KK][4] conductivity fits (ckmi_transport_set_conductivity), else NULL
  double* dfits = nullptr; // device [KK][KK][4] binary diffusion fits (ckmi_transport_set_diffusion), else NULL
  const double* wt = nullptr;  // the mechanism's device weights
  std::vector<double> fits_host;
  std::vector<double> cfits_host;
};
