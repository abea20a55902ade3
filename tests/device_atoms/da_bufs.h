// TEST-ONLY: the device buffers of one harness call (device_atoms28.hip, device_atoms28_points.hip): every entry takes host pointers,
// does its own hipMalloc / copy / ONE launch / sync / copy back and returns the HIP error code; whatever it allocated is freed when
// the call returns, whichever way.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

struct dev_bufs {
  void* p[12];
  int n = 0;
  hipError_t err = hipSuccess;
  ~dev_bufs() {
    for (int i = 0; i < n; i++) (void)hipFree(p[i]);
  }
  template <class T>
  T* in(const T* host, size_t count) {
    T* d = (T*)alloc((count ? count : 1) * sizeof(T));
    if (err == hipSuccess && count) err = hipMemcpy(d, host, count * sizeof(T), hipMemcpyHostToDevice);
    return d;
  }
  template <class T>
  T* out(size_t count) {  // zeroed, so that a lane that wrote nothing shows
    const size_t bytes = (count ? count : 1) * sizeof(T);
    void* d = alloc(bytes);
    if (err == hipSuccess) err = hipMemset(d, 0, bytes);
    return (T*)d;
  }
  void* alloc(size_t bytes) {
    void* d = nullptr;
    if (err == hipSuccess && n == 12) err = hipErrorOutOfMemory;
    if (err == hipSuccess) {
      err = hipMalloc(&d, bytes);
      if (err == hipSuccess) p[n++] = d;
    }
    return d;
  }
  template <class T>
  void back(T* host, const T* d, size_t count) {
    if (err == hipSuccess && count) err = hipMemcpy(host, d, count * sizeof(T), hipMemcpyDeviceToHost);
  }
  void launched() {
    if (err == hipSuccess) err = hipGetLastError();
    if (err == hipSuccess) err = hipDeviceSynchronize();
  }
};

inline unsigned blocks_of(uint32_t n) { return (n + 63u) / 64u; }

}  // namespace
