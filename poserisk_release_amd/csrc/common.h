// Shared host-side helpers for libposerisk_hip.so (gfx950 only; no CUDA/HIP dual paths).
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdlib>

#include "host_common.h"

namespace pr {

#define PR_HIP(call)                                                                      \
  do {                                                                                    \
    hipError_t e__ = (call);                                                              \
    if (e__ != hipSuccess) {                                                              \
      pr::set_error("%s failed: %s (%s:%d)", #call, hipGetErrorString(e__), __FILE__,     \
                    __LINE__);                                                            \
      return PR_ERR_HIP;                                                                  \
    }                                                                                     \
  } while (0)

inline int check_launch(const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    set_error("launch of %s failed: %s", what, hipGetErrorString(e));
    return PR_ERR_HIP;
  }
  return PR_OK;
}

// Raises a kernel's dynamic-LDS limit once per DEVICE (the attribute is per device; a handle may be created on any
// device of the process).  `done` is one word per kernel instantiation, one bit per device ordinal.
inline int ensure_dynamic_lds(const void* kern, size_t bytes, std::atomic<uint64_t>& done) {
  int dev = 0;
  PR_HIP(hipGetDevice(&dev));
  const uint64_t bit = 1ull << (dev & 63);
  if (done.load(std::memory_order_acquire) & bit) return PR_OK;
  PR_HIP(hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
  done.fetch_or(bit, std::memory_order_release);
  return PR_OK;
}

// Capture guard (ABI 10).  pr_*_create, pr_hmr_set_streams and pr_*_destroy allocate, copy and synchronise; reached
// while a stream of the calling thread is being captured into a hipGraph they invalidate the capture, and the process
// aborts at its next synchronisation (round 5, tests: a released SMPL handle re-created inside a capture).  Those entry
// points have no stream argument, so the caller DECLARES the stream it enqueues on (pr_declare_stream, thread-local; the
// Python binding declares torch's current stream); they ask HIP whether it is capturing and return PR_ERR_INVALID,
// having touched nothing.  Entry points that allocate AND take a stream (the stand-alone test entries) check that one.
void declared_stream(bool* declared, hipStream_t* s);
inline int refuse_if_capturing(hipStream_t s, const char* what) {
  hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(s, &st) != hipSuccess) {
    (void)hipGetLastError();   // an invalid or foreign handle says nothing about a capture: not this guard's business
    return PR_OK;
  }
  PR_REQUIRE(st == hipStreamCaptureStatusNone,
             "%s: the caller's stream is being captured into a hipGraph; this call allocates / copies / synchronises and "
             "would invalidate the capture -- create, resize and destroy handles outside the capture", what);
  return PR_OK;
}
inline int refuse_under_declared_capture(const char* what) {
  bool declared = false;
  hipStream_t s = nullptr;
  declared_stream(&declared, &s);
  return declared ? refuse_if_capturing(s, what) : PR_OK;
}

// RAII device selection for create/destroy paths.
struct DeviceGuard {
  int prev = -1;
  bool ok = false;
  explicit DeviceGuard(int dev) {
    if (hipGetDevice(&prev) == hipSuccess && hipSetDevice(dev) == hipSuccess) ok = true;
  }
  ~DeviceGuard() {
    if (prev >= 0) (void)hipSetDevice(prev);
  }
};

// Compute units of the current device, asked once per device (the persistent kernels size their grids by it at every launch).
inline int current_device_cus(int* cus) {
  static std::atomic<int> cache[64] = {};
  int dev = 0;
  PR_HIP(hipGetDevice(&dev));
  int n = cache[dev & 63].load(std::memory_order_relaxed);
  if (!n) {
    PR_HIP(hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev));
    if (n <= 0) n = 256;
    cache[dev & 63].store(n, std::memory_order_relaxed);
  }
  *cus = n;
  return PR_OK;
}

}  // namespace pr
