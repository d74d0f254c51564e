// Host-side helpers that need no HIP header: the error state and the status macros.  Included by common.h (device
// translation units) and by host_plan.cc, which is also compiled WITHOUT the HIP toolchain for the sanitizer build of
// tests/native (g++ -fsanitize=address,undefined).
#pragma once
#include <cstdarg>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>

#include "../../include/poserisk_hip.h"

namespace pr {

void set_error(const char* fmt, ...);

#define PR_REQUIRE(cond, ...)        \
  do {                               \
    if (!(cond)) {                   \
      pr::set_error(__VA_ARGS__);    \
      return PR_ERR_INVALID;         \
    }                                \
  } while (0)

#define PR_TRY(expr)             \
  do {                           \
    int s__ = (expr);            \
    if (s__ != PR_OK) return s__; \
  } while (0)

inline int ceil_div(int a, int b) { return (a + b - 1) / b; }
inline long ceil_div(long a, long b) { return (a + b - 1) / b; }
inline int ilog2_exact(int v) {   // log2 of a power of two, -1 for anything else
  int l = 0;
  while ((1 << l) < v) ++l;
  return (1 << l) == v ? l : -1;
}

// ---- the internal fence's device-free part (fence.h has the allocator; DESIGN.md "The internal fence") ----------------
// POSERISK_FENCE=1 | 2 turns every device allocation of the library's own into guard | payload | guard, all 0xFF bytes
// (NaN as fp32 and as bf16, -1 as int32) before use.  A guard is at least 64 KiB and at least one frame of the largest
// tensor its buffer holds, rounded up to 4096 bytes so that the payload keeps the device allocator's alignment.
constexpr size_t kFenceMinGuard = (size_t)64 << 10;
constexpr size_t kFenceGuardAlign = 4096;
constexpr size_t kFenceTensorAlign = 256;
constexpr unsigned char kFenceFill = 0xFF;
inline size_t fence_guard_bytes(size_t frame_bytes) {
  const size_t g = frame_bytes > kFenceMinGuard ? frame_bytes : kFenceMinGuard;
  return (g + kFenceGuardAlign - 1) / kFenceGuardAlign * kFenceGuardAlign;
}
// Mode 2 (tail): a tensor of `tensor_bytes` in a buffer of `capacity_bytes` ends on the buffer's last byte.  *ok = false
// where it does not fit or its size is no multiple of 256 bytes (the offset then misaligns the tensor): the offset returned
// is still inside the buffer and the same for every caller with the same dimensions, the caller reports the failure.
inline size_t fence_tail_offset(size_t capacity_bytes, size_t tensor_bytes, bool* ok) {
  if (tensor_bytes > capacity_bytes) {
    *ok = false;
    return 0;
  }
  if (tensor_bytes % kFenceTensorAlign != 0 || capacity_bytes % kFenceTensorAlign != 0) *ok = false;
  return capacity_bytes - tensor_bytes;
}
// Bytes of a host copy of a guard that are no longer 0xFF: how many, the first and the last (indices into `guard`).
struct FenceScan {
  size_t count = 0, first = 0, last = 0;
};
inline FenceScan fence_scan(const unsigned char* guard, size_t n) {
  FenceScan s;
  for (size_t i = 0; i < n; ++i)
    if (guard[i] != kFenceFill) {
      if (!s.count) s.first = i;
      s.last = i;
      ++s.count;
    }
  return s;
}

}  // namespace pr
