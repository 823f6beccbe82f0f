// How a C entry launches a kernel: one_of (dispatch.h) picks the template arguments, launch() runs
// it and reports, resident_workgroups() sizes a persistent grid.
#pragma once
#include "common.h"
#include "dispatch.h"

// kernel<<<grid, block, 0, stream>>>(args...), the error left for last_error(). A kernel's default
// arguments do not travel with its address: pass every argument.
template <class... P, class... A>
inline void enqueue(void (*kernel)(P...), dim3 grid, dim3 block, hipStream_t stream, A&&... args) {
  hipLaunchKernelGGL(kernel, grid, block, 0, stream, std::forward<A>(args)...);
}
// LGNN_OK, or the HIP error code the calls since the last reading left behind
inline int last_error() {
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? LGNN_OK : (int)e;
}
// One launch and its result. Several launches that report once (the GAT strip loops) are
// enqueue() ... enqueue(), return last_error().
template <class... P, class... A>
inline int launch(void (*kernel)(P...), dim3 grid, dim3 block, hipStream_t stream, A&&... args) {
  enqueue(kernel, grid, block, stream, std::forward<A>(args)...);
  return last_error();
}
// The same with `lds` bytes of dynamic LDS.
template <class... P, class... A>
inline int launch_lds(void (*kernel)(P...), dim3 grid, dim3 block, size_t lds, hipStream_t stream,
                      A&&... args) {
  hipLaunchKernelGGL(kernel, grid, block, lds, stream, std::forward<A>(args)...);
  return last_error();
}

// The residency caches below hold devices 0..15; a device index beyond that is served by the same
// queries, uncached.
constexpr int LGNN_CACHED_DEVICES = 16;

inline int current_device() {
  int dev = -1;
  return hipGetDevice(&dev) == hipSuccess ? dev : -1;
}

// Compute units of device dev; 0 when the query fails. Asked once per device: the outcome is
// cached, a failure too.
inline int device_cus(int dev) {
  static int cache[LGNN_CACHED_DEVICES];
  static bool have[LGNN_CACHED_DEVICES];
  const bool keep = dev >= 0 && dev < LGNN_CACHED_DEVICES;
  if (keep && have[dev]) return cache[dev];
  int cus = 0;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess ||
      cus < 0)
    cus = 0;
  if (keep) cache[dev] = cus, have[dev] = true;
  return cus;
}
// ... of the current device
inline int device_cus() { return device_cus(current_device()); }

// Workgroups of `threads` threads of kernel K that one CU of the current device keeps resident,
// cached per (device, kernel): the static belongs to this instantiation, so the kernel itself is
// the key. dev is the current device's index (the cache key; the query is the runtime's, of the
// current device). A negative value is a HIP error code, negated. Asked once: the outcome is
// cached, a zero or a failure too.
template <auto K>
inline int workgroups_per_cu(int threads, int dev) {
  static int cache[LGNN_CACHED_DEVICES];
  static bool have[LGNN_CACHED_DEVICES];
  const bool keep = dev >= 0 && dev < LGNN_CACHED_DEVICES;
  if (keep && have[dev]) return cache[dev];
  int per = 0;
  const hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per, K, threads, 0);
  if (e != hipSuccess) per = -(int)e;
  if (keep) cache[dev] = per, have[dev] = true;
  return per;
}

// Workgroups of kernel K resident on the current device at once: occupancy per CU x CUs.
// Negative: a HIP error code, negated.
template <auto K>
inline int resident_workgroups(int threads, int dev) {
  const int cus = device_cus(dev);
  if (cus <= 0) return -(int)hipErrorInvalidDevice;
  const int per = workgroups_per_cu<K>(threads, dev);
  return per < 0 ? per : cus * per;
}
template <auto K>
inline int resident_workgroups(int threads) {
  return resident_workgroups<K>(threads, current_device());
}
