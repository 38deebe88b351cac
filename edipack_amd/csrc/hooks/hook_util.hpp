// hook_util.hpp -- what the test hooks of this directory share: whole-buffer device copies of host buffers given as
// pointer + length in doubles, the refusal with a message, the device check and the final synchronisation.
#pragma once
#include <algorithm>
#include <string>

#include "../dev_mem.hpp"
#include "../kernels.hpp"

namespace edigpu {
namespace {

struct DevBuf {
  double* p = nullptr;
  size_t n = 0;
  ~DevBuf() { dev_free(p); }
  int up(const double* h, int64_t len) {
    n = (size_t)len;
    EDIGPU_HIP(hipMalloc((void**)&p, std::max<size_t>(n, 1) * sizeof(double)));
    if (n) EDIGPU_HIP(hipMemcpy(p, h, n * sizeof(double), hipMemcpyHostToDevice));
    return 0;
  }
  int alloc(size_t cnt) {  // scratch: never downloaded
    EDIGPU_HIP(hipMalloc((void**)&p, std::max<size_t>(cnt, 1) * sizeof(double)));
    return 0;
  }
  int down(double* h) const {
    if (n) EDIGPU_HIP(hipMemcpy(h, p, n * sizeof(double), hipMemcpyDeviceToHost));
    return 0;
  }
};

struct DevInt {
  int* p = nullptr;
  ~DevInt() { dev_free(p); }
  int up(int v) {
    EDIGPU_HIP(hipMalloc((void**)&p, sizeof(int)));
    EDIGPU_HIP(hipMemcpy(p, &v, sizeof(int), hipMemcpyHostToDevice));
    return 0;
  }
  int down(int* v) const {
    EDIGPU_HIP(hipMemcpy(v, p, sizeof(int), hipMemcpyDeviceToHost));
    return 0;
  }
};

[[maybe_unused]] int refuse(const char* who, const char* what) {
  set_error(std::string(who) + ": " + what);
  return 1;
}

[[maybe_unused]] int need_device() {
  int n = 0;
  return edigpu_device_count(&n);  // sets the message
}

[[maybe_unused]] int finish(const char* who) {
  if (hipDeviceSynchronize() != hipSuccess) return refuse(who, "the kernel failed");
  return 0;
}

}  // namespace
}  // namespace edigpu
