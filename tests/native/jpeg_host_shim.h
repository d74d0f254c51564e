// Stands in for csrc/common.h when csrc/jpeg.hip is compiled for the HOST (tests/test_jpeg_native.py copies both into one
// directory, this file as common.h).  The decoder's kernels index by thread only -- no LDS, no barrier, no cross-lane operation
// -- so a launch is two nested loops: workgroups one after the other, their threads one after the other.  The bit reader, the
// Huffman tables' indexing, the coefficient scatter, the IDCT's 32-bit arithmetic and every address the kernels form then run
// under AddressSanitizer and UndefinedBehaviorSanitizer against exact-size heap buffers.  Nothing here is GPU code.
#pragma once
#include <algorithm>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "host_common.h"

struct dim3 {
  unsigned x, y, z;
  dim3(unsigned a = 1, unsigned b = 1, unsigned c = 1) : x(a), y(b), z(c) {}
};
typedef void* hipStream_t;

inline dim3 threadIdx, blockIdx;
using std::max;
using std::min;
inline int atomicOr(int* p, int v) {
  const int old = *p;
  *p = old | v;
  return old;
}
inline int hipMemsetAsync(void* p, int v, size_t n, hipStream_t) {
  memset(p, v, n);
  return 0;
}

#define __global__
#define __device__
#define __forceinline__ inline
#define __launch_bounds__(x)
#define PR_HIP(call) \
  do {               \
    (void)(call);    \
  } while (0)

template <class Kernel, class Params>
void launch_on_host(Kernel kernel, dim3 grid, dim3 block, Params p) {
  for (unsigned by = 0; by < grid.y; ++by)
    for (unsigned bx = 0; bx < grid.x; ++bx)
      for (unsigned t = 0; t < block.x; ++t) {
        blockIdx = dim3(bx, by);
        threadIdx = dim3(t);
        kernel(p);
      }
}
#define hipLaunchKernelGGL(kernel, grid, block, lds_bytes, stream, p) launch_on_host(kernel, grid, block, p)

namespace pr {
inline int check_launch(const char*) { return PR_OK; }
inline int current_device_cus(int* cus) {   // a small machine: the entropy kernel then packs several segments into a wave
  *cus = 1;
  return PR_OK;
}
}  // namespace pr
