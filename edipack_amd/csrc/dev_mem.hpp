// dev_mem.hpp -- the device-memory helpers of the C-ABI layer: upload, allocate, free, grow.  Every one returns 0, or 1 with the
// message set (EDIGPU_HIP).
#pragma once
#include <vector>

#include "edigpu_internal.hpp"

namespace edigpu {

// *d = a fresh device copy of h[0:n]; null when n == 0
template <class T>
int dev_upload(T** d, const T* h, size_t n) {
  *d = nullptr;
  if (n == 0) return 0;
  EDIGPU_HIP(hipMalloc((void**)d, n * sizeof(T)));
  EDIGPU_HIP(hipMemcpy(*d, h, n * sizeof(T), hipMemcpyHostToDevice));
  return 0;
}

template <class T>
int dev_upload(T** out, const std::vector<T>& h) {
  return dev_upload(out, h.data(), h.size());
}

template <class T>
void dev_free(T*& p) {  // (T may be const: the kernels' argument blocks hold pointers to const)
  if (p) (void)hipFree((void*)p);
  p = nullptr;
}

template <class... T>
void dev_free_all(T*&... p) {
  (dev_free(p), ...);
}

// a buffer of at least `need` elements, its capacity kept in *cap: nothing to do when it is large enough, else free and
// allocate anew (the contents are lost).  When the allocation fails the buffer is null and the capacity zero.
template <class T, class N>
int dev_grow(T** d, N* cap, N need) {
  if (*cap >= need) return 0;
  dev_free(*d);
  *cap = 0;
  EDIGPU_HIP(hipMalloc((void**)d, (size_t)need * sizeof(T)));
  *cap = need;
  return 0;
}

#pragma GCC visibility push(hidden)
// *d = a fresh buffer of n elements (of one when n == 0), contents undefined
template <class T>
int dev_alloc(T** d, size_t n) {
  *d = nullptr;
  EDIGPU_HIP(hipMalloc((void**)d, (n > 0 ? n : 1) * sizeof(T)));
  return 0;
}

// p = a fresh buffer of n elements (of one when n == 0) that holds zeros once this returns: the old one is freed, the new
// one is zeroed on the null stream and the DEVICE is synchronised, since the handles' non-blocking streams do not wait
// for the null stream
template <class T>
int dev_realloc_zeroed_sync(T*& p, size_t n) {
  dev_free(p);
  if (dev_alloc(&p, n)) return 1;
  EDIGPU_HIP(hipMemset(p, 0, (n > 0 ? n : 1) * sizeof(T)));
  EDIGPU_HIP(hipDeviceSynchronize());
  return 0;
}
#pragma GCC visibility pop

}  // namespace edigpu
