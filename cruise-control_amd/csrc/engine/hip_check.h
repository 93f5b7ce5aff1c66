// hipCheck and DeviceGuard for the translation units that call the HIP runtime (device.cpp, device_accept.cpp and the
// aggregator family: ccmi_aggregator.cpp, ccmi_load_model.cpp, ccmi_anomaly.cpp). Owning device and pinned memory is
// not done here: devbuf.h has the buffers, device.cpp the four HIP calls behind them. Product only: the test emulation
// of Device has no HIP and does not include this.
#pragma once
#include <hip/hip_runtime.h>

#include <stdexcept>
#include <string>

namespace ccmi {

inline void hipCheck(hipError_t e, const char* what) {
  if (e != hipSuccess) throw std::runtime_error(std::string("HIP error in ") + what + ": " + hipGetErrorString(e));
}

// HIP's current device is per host thread and starts at 0; a session may run on a thread other than the one that
// created it (the reference's precompute pool, bench.py --requests-per-gpu). Every public entry point that touches
// the device makes the session's ordinal current for its duration and restores the caller's device afterwards.
struct DeviceGuard {
  int prev = -1;
  explicit DeviceGuard(int ordinal) {
    hipCheck(hipGetDevice(&prev), "hipGetDevice");
    if (prev != ordinal) hipCheck(hipSetDevice(ordinal), "hipSetDevice");
    else prev = -1;
  }
  ~DeviceGuard() {
    if (prev >= 0) (void)hipSetDevice(prev);
  }
};

}  // namespace ccmi
