// ckmi_internal.hpp -- host-side internals shared by the translation units of libckmi.so.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/ckmi.h"
#include "ckmi_device.hpp"
#include "ckmi_dispatch.hpp"
#include "ckmi_image.hpp"
#include "ckmi_mech_host.hpp"

namespace ckmi {
// mechanism-specialised ROP kernel (ckmi_jit.cpp): source generated at ckmi_mech_create, compiled
// with hipRTC at the first call that selects it
struct JitRop {
  std::string src, why;
  std::vector<int> lnA_off;  // original reaction -> offset of its ln A in the parameter block
  double* prm = nullptr;     // device parameter block
  std::atomic<int> state{0};  // 0 not compiled yet, 1 ready, -1 unsupported / compile failed (why, under mu)
  hipModule_t mod = nullptr;
  hipFunction_t fn = nullptr;
  std::mutex mu;
};
bool jit_rop_generate(const ckmi_mech_desc* d, std::string& src, std::vector<double>& prm, std::vector<int>& lnA_off,
                      std::string& why);
int jit_rop_compile(const std::string& src, std::vector<char>& code, std::string& log);
}  // namespace ckmi

// The mechanism handle: what build_host_mech derived (sizes, maps, host copies; img with its device pointers
// set once uploaded) and the device copies ckmi_mech_create made of it.
struct ckmi_mech : ckmi::HostMech {
  int device = 0;
  ckmi::MechDev d{};            // species tables in global memory
  const int* d_orig = nullptr;  // device copy of orig (rop_kernel writes rates in the original order)
  std::vector<void*> allocs;
  ckmi::JitRop* jit = nullptr;
  // equilibrium tables (ckmi_equil.hip): [KK][EQ_ROW] built from the image at the first ckmi_equil_run and
  // owned by allocs; eq_mm = 0 until then
  const double* eq_tab = nullptr;
  int eq_mm = 0;
};

namespace ckmi {
struct DevCfg;
struct ReactorIO;
struct ProbeIO;
struct NewtonProbeIO;
#define CKMI_HIP_CHECK(x)                                                                                        \
  do {                                                                                                           \
    hipError_t e_ = (x);                                                                                         \
    if (e_ != hipSuccess) return ckmi::set_error(CKMI_ERR_HIP, std::string(#x) + ": " + hipGetErrorString(e_)); \
  } while (0)

// ---------------------------------------------------------------- the launch layer (ckmi.hip)
// The stream-ordered workspace of one launch or call: one hipMallocAsync, released behind the work on every
// way out, handed out front to back in 256-byte-aligned pieces.
class StreamWorkspace {
 public:
  explicit StreamWorkspace(hipStream_t stream) : st_(stream) {}
  ~StreamWorkspace() {
    if (base_) (void)hipFreeAsync(base_, st_);
  }
  StreamWorkspace(const StreamWorkspace&) = delete;
  StreamWorkspace& operator=(const StreamWorkspace&) = delete;
  static constexpr size_t aligned(size_t bytes) { return (bytes + 255) & ~(size_t)255; }
  int alloc(size_t bytes) {
    CKMI_HIP_CHECK(hipMallocAsync((void**)&base_, bytes, st_));
    return CKMI_OK;
  }
  // the next piece; bytes is rounded up to the alignment
  template <class T>
  T* take(size_t bytes) {
    T* p = (T*)(base_ + off_);
    off_ += aligned(bytes);
    return p;
  }

 private:
  hipStream_t st_;
  char* base_ = nullptr;
  size_t off_ = 0;
};
// Per-launch copy of the run configuration: it lives in the launch's stream-ordered workspace, so launches with
// different configurations on one mechanism handle (other streams, other host threads) never share it.  The
// host staging copy is released by a host function enqueued behind the copy, i.e. only once the stream has
// consumed it.
int stage_cfg(const DevCfg& dc, DevCfg* dst, hipStream_t stream);
// raise fn's dynamic-LDS limit on device to bytes: above the 64 KiB every kernel has, and only ever upwards
int raise_lds_limit(int device, const void* fn, size_t bytes);
// The device configuration of a call: GFAC 0 -> 1 and the runaway guard; integrate (a closed-reactor run) adds
// the profile breakpoints and the element projection, which the probes, the heat rates and the open reactor
// (it relaxes to the inlet's element content, not the estimate's) leave off.
DevCfg make_dev_cfg(const ckmi_mech* m, const ckmi_reactor_cfg* cfg, bool integrate);
// what ckmi_reactor_run_ex, ckmi_psr_run and ckmi_reactor_rhs_jac all require of a configuration; profiles:
// the entry takes profiles (an open reactor refuses them itself and never reads their kinds)
int check_reactor_cfg(const ckmi_reactor_cfg* cfg, const ckmi_reactor_ext* ext, bool profiles);

// one workgroup per reactor: 64 <= KK + 1 <= 192 (ckmi_big.hip)
int launch_big_reactors(const ckmi_mech* m, int n, const DevCfg& dc, const ReactorIO& io, hipStream_t stream);
// RHS / Jacobian probes of ckmi_reactor_rhs_jac: the workgroup kernel's (ckmi_big.hip) and the open-reactor
// instantiation of the wave kernel's (ckmi_psr.hip)
int launch_big_probe(const ckmi_mech* m, int n, const DevCfg& dc, const ProbeIO& io, hipStream_t stream);
int launch_psr_probe(const ckmi_mech* m, int n, const DevCfg& dc, const ProbeIO& io, hipStream_t stream);
// Newton-matrix probe of ckmi_newton_probe on the workgroup kernel's BigMat<NB> (ckmi_big.hip)
int launch_big_newton_probe(int NB, const NewtonProbeIO& io, hipStream_t stream);
}  // namespace ckmi
