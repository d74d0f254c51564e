// Stands in for csrc/common.h when a kernel file (compose.hip, jpeg*.hip, resize.hip, yuv*.hip) is compiled for the HOST:
// tests/host_build.py copies the kernel files and this file, as common.h, into one directory.  The kernels' index arithmetic,
// their rounding and every address they form then run under ASan and UBSan against exact-size
// heap buffers.  Nothing here is GPU code.  A launch walks grid.y, grid.x and block.x in nested loops, workgroups one after the
// other, their threads one after the other: right for kernels that index by thread only.  Two macros, defined by the driver
// before its first include, change that; there are no other switches.
//   HOST_SHIM_THREADS   a workgroup is block.x host threads and __syncthreads a barrier (compose.hip); workgroups still run one
//                       after the other.  Without it __syncthreads does not exist and a kernel that calls it does not compile.
//   HOST_SHIM_SHARED    what __shared__ expands to.  Default `static`: a fixed LDS array of which each lane touches its own
//                       slice (jpeg_scans.hip).  Empty for compose.hip's `extern __shared__` block, which the driver defines
//                       as a global array of kLdsBytes.
#pragma once
#include <algorithm>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#ifdef HOST_SHIM_THREADS
#include <condition_variable>
#include <mutex>
#include <thread>
#include <vector>
#endif

#include "host_common.h"

struct dim3 {
  unsigned x, y, z;
  constexpr dim3(unsigned a = 1, unsigned b = 1, unsigned c = 1) : x(a), y(b), z(c) {}
};
struct uint4 {
  unsigned x, y, z, w;
};
inline uint4 make_uint4(unsigned a, unsigned b, unsigned c, unsigned d) { return uint4{a, b, c, d}; }
typedef void* hipStream_t;

inline thread_local dim3 threadIdx, blockIdx;
using std::max;
using std::min;
inline float __uint2float_rn(unsigned v) { return (float)v; }
inline int atomicOr(int* p, int v) { return __atomic_fetch_or(p, v, __ATOMIC_SEQ_CST); }
inline unsigned atomicOr(unsigned* p, unsigned v) { return __atomic_fetch_or(p, v, __ATOMIC_SEQ_CST); }
inline int atomicAdd(int* p, int v) { return __atomic_fetch_add(p, v, __ATOMIC_SEQ_CST); }
inline unsigned atomicAdd(unsigned* p, unsigned v) { return __atomic_fetch_add(p, v, __ATOMIC_SEQ_CST); }
template <class T>
inline T atomicMax(T* p, T v) {
  T old = __atomic_load_n(p, __ATOMIC_SEQ_CST);
  while (old < v && !__atomic_compare_exchange_n(p, &old, v, false, __ATOMIC_SEQ_CST, __ATOMIC_SEQ_CST)) {
  }
  return old;
}
inline int hipMemsetAsync(void* p, int v, size_t n, hipStream_t) {
  memset(p, v, n);
  return 0;
}

constexpr size_t kLdsBytes = 64 * 1024;          // what a workgroup may have without raising the limit
inline size_t g_lds_asked = 0;                   // the largest dynamic LDS block any launch asked for

#ifndef HOST_SHIM_SHARED
#define HOST_SHIM_SHARED static
#endif
#define __global__
#define __device__
#define __forceinline__ inline
#define __launch_bounds__(x)
#define __shared__ HOST_SHIM_SHARED
#define PR_HIP(call) \
  do {               \
    (void)(call);    \
  } while (0)

#ifdef HOST_SHIM_THREADS
class Barrier {
 public:
  explicit Barrier(unsigned n) : n_(n) {}
  void wait() {
    std::unique_lock<std::mutex> l(m_);
    const unsigned gen = gen_;
    if (++count_ == n_) {
      count_ = 0;
      ++gen_;
      cv_.notify_all();
    } else {
      cv_.wait(l, [&] { return gen != gen_; });
    }
  }

 private:
  std::mutex m_;
  std::condition_variable cv_;
  unsigned n_, count_ = 0, gen_ = 0;
};
inline Barrier* g_barrier = nullptr;
inline void __syncthreads() { g_barrier->wait(); }
#endif

template <class Kernel, class Params>
void launch_on_host(Kernel kernel, dim3 grid, dim3 block, size_t lds_bytes, Params p) {
  g_lds_asked = std::max(g_lds_asked, lds_bytes);
#ifdef HOST_SHIM_THREADS
  Barrier barrier(block.x);
  g_barrier = &barrier;
  std::vector<std::thread> threads;
  for (unsigned t = 0; t < block.x; ++t)
    threads.emplace_back([=, &barrier] {
      for (unsigned by = 0; by < grid.y; ++by)
        for (unsigned bx = 0; bx < grid.x; ++bx) {
          threadIdx = dim3(t);
          blockIdx = dim3(bx, by);
          kernel(p);
          barrier.wait();          // the next workgroup reuses the LDS block
        }
    });
  for (auto& t : threads) t.join();
#else
  for (unsigned by = 0; by < grid.y; ++by)
    for (unsigned bx = 0; bx < grid.x; ++bx)
      for (unsigned t = 0; t < block.x; ++t) {
        blockIdx = dim3(bx, by);
        threadIdx = dim3(t);
        kernel(p);
      }
#endif
}
#define hipLaunchKernelGGL(kernel, grid, block, lds_bytes, stream, p) launch_on_host(kernel, grid, block, lds_bytes, p)

namespace pr {
inline int check_launch(const char*) { return PR_OK; }
inline int current_device_cus(int* cus) {   // a small machine: the entropy kernels then pack several segments into a wave
  *cus = 1;
  return PR_OK;
}
}  // namespace pr
