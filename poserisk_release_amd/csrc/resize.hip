// Device half of the frame downscale: u8[F,H,W,3] -> u8[F,h,w,3] by the integer bilinear contract of include/poserisk_hip.h
// (section j3).  The tap tables come from pr_resize_plan (csrc/resize_host.cc); tests/resize_ref.py restates the contract in
// numpy, tests/test_frontend_native.py runs this file on the host under sanitizers, tests/test_frontend_gpu.py on the device.
//
// The output of a call is one flat run of F * h * w * 3 bytes.  h * w * 3 need not be a multiple of 4, so a frame after the
// first may start at any alignment: the kernel does not work frame by frame but in ALIGNED DWORDS of that flat run.  Lane g
// owns the g-th aligned dword (four consecutive output bytes, which may straddle a row's or a frame's end: each byte finds its
// own frame, row, column and channel) and stores it once; the up to three bytes in front of the first aligned dword and the
// up to three behind the last are stored byte by byte by up to six lanes behind the others.  Consecutive lanes hold
// consecutive output bytes of one row, so a wave stores 256 contiguous bytes and its loads walk two source rows in order:
// each 128-byte line of a source row is fetched by one wave, about 2.4 of them per load instruction at 1920 -> 800.
// The tables are a few KB and stay in L1 / L2.
// Kernels index by thread only: no LDS, no barrier, no cross-lane operation, plain C++ and vector memory operations.
#include "common.h"

namespace pr {
namespace {

constexpr int kResizeThreads = 256;

struct ResizeParams {
  const uint8_t* src;
  uint8_t* dst;
  const int32_t* xofs;
  const int16_t* xcoef;
  const int32_t* yofs;
  const int16_t* ycoef;
  int H, W, h, w, mode;
  int row_bytes;       // w * 3
  int frame_bytes;     // h * w * 3
  int head;            // bytes in front of the first aligned dword of dst: 0..3 (the whole call when it is shorter)
  long total;          // F * h * w * 3
  long dwords;         // aligned dwords of the call
};

// The output byte at (frame f, row y, byte cb of the row).
__device__ __forceinline__ unsigned resize_byte(const ResizeParams& p, long f, int y, int cb) {
  const uint8_t* s = p.src + f * ((long)p.H * p.W * 3);
  if (p.mode == PR_RESIZE_COPY) return s[(long)y * p.row_bytes + cb];
  const int x = cb / 3, c = cb - 3 * x;
  const long pitch = (long)p.W * 3;
  if (p.mode == PR_RESIZE_HALF) {
    const uint8_t* q = s + (long)(2 * y) * pitch + 6 * x + c;
    return (unsigned)(q[0] + q[3] + q[pitch] + q[pitch + 3] + 2) >> 2;
  }
  // the plan's offsets lie in 0..S-1; clamped all the same, so that no table content can form an address outside src
  const int x0 = min(max(p.xofs[x], 0), p.W - 1), x1 = min(x0 + 1, p.W - 1);
  const int y0 = min(max(p.yofs[y], 0), p.H - 1), y1 = min(y0 + 1, p.H - 1);
  const int a0 = p.xcoef[2 * x], a1 = p.xcoef[2 * x + 1], b0 = p.ycoef[2 * y], b1 = p.ycoef[2 * y + 1];
  const uint8_t* r0 = s + y0 * pitch + c;
  const uint8_t* r1 = s + y1 * pitch + c;
  const int t0 = r0[3 * x0] * a0 + r0[3 * x1] * a1, t1 = r1[3 * x0] * a0 + r1[3 * x1] * a1;
  return (unsigned)((((b0 * (t0 >> 4)) >> 16) + ((b1 * (t1 >> 4)) >> 16) + 2) >> 2);
}

__global__ void __launch_bounds__(kResizeThreads) resize_frames_kernel(ResizeParams p) {
  const long g = (long)blockIdx.x * kResizeThreads + threadIdx.x;
  int count = 4;
  long n;                                             // the lane's first byte in the flat output
  if (g < p.dwords) {
    n = p.head + 4 * g;
  } else {                                            // the unaligned ends: one byte a lane
    const long e = g - p.dwords;
    const long tail0 = p.head + 4 * p.dwords;
    n = e < p.head ? e : tail0 + (e - p.head);
    if (n >= p.total) return;
    count = 1;
  }
  const long f0 = n / p.frame_bytes;
  const int rem = (int)(n - f0 * p.frame_bytes);
  long f = f0;
  int y = rem / p.row_bytes, cb = rem - y * p.row_bytes;
  if (count == 1) {
    p.dst[n] = (uint8_t)resize_byte(p, f, y, cb);
    return;
  }
  unsigned word = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    word |= resize_byte(p, f, y, cb) << (8 * k);
    if (++cb == p.row_bytes) {
      cb = 0;
      if (++y == p.h) y = 0, ++f;
    }
  }
  __builtin_memcpy(__builtin_assume_aligned(p.dst + n, 4), &word, 4);
}

}  // namespace
}  // namespace pr

extern "C" int pr_resize_frames(const uint8_t* src, int F, int H, int W, uint8_t* dst, int h, int w, const int32_t* xofs,
                                const int16_t* xcoef, const int32_t* yofs, const int16_t* ycoef, int mode, void* stream) {
  using namespace pr;
  PR_REQUIRE(F >= 0, "pr_resize_frames: F = %d", F);
  if (F == 0) return PR_OK;
  PR_REQUIRE(H >= 1 && H <= PR_RESIZE_MAX_SIDE && W >= 1 && W <= PR_RESIZE_MAX_SIDE && h >= 1 && h <= PR_RESIZE_MAX_SIDE &&
                 w >= 1 && w <= PR_RESIZE_MAX_SIDE,
             "pr_resize_frames: %d x %d -> %d x %d: every side must lie in 1..%d", W, H, w, h, PR_RESIZE_MAX_SIDE);
  const int want = (H == h && W == w) ? PR_RESIZE_COPY : (W == 2 * w && H == 2 * h) ? PR_RESIZE_HALF : PR_RESIZE_LINEAR;
  PR_REQUIRE(mode == want, "pr_resize_frames: mode = %d, but %d x %d -> %d x %d is mode %d (pass what pr_resize_plan gave)", mode,
             W, H, w, h, want);
  PR_REQUIRE(src, "pr_resize_frames: null src");
  PR_REQUIRE(dst, "pr_resize_frames: null dst");
  PR_REQUIRE(xofs, "pr_resize_frames: null xofs");
  PR_REQUIRE(xcoef, "pr_resize_frames: null xcoef");
  PR_REQUIRE(yofs, "pr_resize_frames: null yofs");
  PR_REQUIRE(ycoef, "pr_resize_frames: null ycoef");
  ResizeParams p;
  p.src = src;
  p.dst = dst;
  p.xofs = xofs;
  p.xcoef = xcoef;
  p.yofs = yofs;
  p.ycoef = ycoef;
  p.H = H, p.W = W, p.h = h, p.w = w, p.mode = mode;
  p.row_bytes = w * 3;
  p.frame_bytes = h * w * 3;
  p.total = (long)F * p.frame_bytes;
  p.head = (int)std::min<long>((long)(-(uintptr_t)dst & 3), p.total);
  p.dwords = (p.total - p.head) / 4;
  const long lanes = p.dwords + 6;                   // the ends take at most 3 + 3 lanes
  const long blocks = ceil_div(lanes, (long)kResizeThreads);
  PR_REQUIRE(blocks <= 0x7fffffffl, "pr_resize_frames: %d frames of %d x %d are too many bytes for one call", F, w, h);
  hipLaunchKernelGGL(resize_frames_kernel, dim3((unsigned)blocks), dim3(kResizeThreads), 0, (hipStream_t)stream, p);
  return check_launch("resize_frames_kernel");
}
