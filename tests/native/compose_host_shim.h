// Stands in for csrc/common.h when csrc/compose.hip is compiled for the HOST (tests/test_video_native.py copies both into one
// directory, this file as common.h): a workgroup is 256 host threads, __syncthreads a barrier, the dynamic LDS block a global
// array, workgroups run one after the other.  The kernel's index arithmetic, its rounding and every address it forms then run
// under AddressSanitizer and UndefinedBehaviorSanitizer against exact-size heap buffers.  Nothing here is GPU code.
#pragma once
#include <algorithm>
#include <condition_variable>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <thread>
#include <vector>

#include "host_common.h"

struct dim3 {
  unsigned x, y, z;
  dim3(unsigned a = 1, unsigned b = 1, unsigned c = 1) : x(a), y(b), z(c) {}
};
struct uint4 {
  unsigned x, y, z, w;
};
inline uint4 make_uint4(unsigned a, unsigned b, unsigned c, unsigned d) { return uint4{a, b, c, d}; }
typedef void* hipStream_t;

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

inline thread_local dim3 threadIdx, blockIdx;
inline Barrier* g_barrier = nullptr;
inline void __syncthreads() { g_barrier->wait(); }
using std::max;
using std::min;
inline float __uint2float_rn(unsigned v) { return (float)v; }
inline unsigned atomicOr(unsigned* p, unsigned v) { return __atomic_fetch_or(p, v, __ATOMIC_SEQ_CST); }

constexpr size_t kLdsBytes = 64 * 1024;          // what a workgroup may have without raising the limit
extern unsigned pr_compose_lds[];
inline size_t g_lds_asked = 0;

#define __global__
#define __device__
#define __forceinline__ inline
#define __launch_bounds__(x)
#define __shared__

template <class Kernel, class Params>
void launch_on_host(Kernel kernel, dim3 grid, dim3 block, size_t lds_bytes, Params p) {
  g_lds_asked = std::max(g_lds_asked, lds_bytes);
  Barrier barrier(block.x);
  g_barrier = &barrier;
  std::vector<std::thread> threads;
  for (unsigned t = 0; t < block.x; ++t)
    threads.emplace_back([=, &barrier] {
      for (unsigned b = 0; b < grid.x; ++b) {
        threadIdx = dim3(t);
        blockIdx = dim3(b);
        kernel(p);
        barrier.wait();          // the next workgroup reuses the LDS block
      }
    });
  for (auto& t : threads) t.join();
}
#define hipLaunchKernelGGL(kernel, grid, block, lds_bytes, stream, p) launch_on_host(kernel, grid, block, lds_bytes, p)

namespace pr {
inline int check_launch(const char*) { return PR_OK; }
}  // namespace pr
