// Device half of the YUV4MPEG2 reader: the raw planes of a chunk of the stream -> u8[F,h,w,3] by the contract of
// include/poserisk_hip.h (section j6): chroma to full resolution at a scale of 16, the integer colour matrix and, with the
// tables of pr_resize_plan given, j3's downscale of that RGB -- in one kernel, so that the source-size RGB is never written.
// tests/yuv_ref.py restates the contract in numpy, tests/test_y4m_native.py runs this file on the host under sanitizers,
// tests/test_y4m_gpu.py on the device.
//
// As in resize.hip the output of a call is one flat run of F * h * w * 3 bytes written in ALIGNED DWORDS, but three of them a
// lane: 12 bytes are four whole pixels where dst is 4-byte aligned (a pixel boundary is every third byte of the flat run,
// whatever the frame and row sizes), five where it is not.  A lane computes each of its output pixels once, all three
// channels from one set of loads, packs them into a 128-bit register, shifts the run to its first byte and stores it
// once; the up to three bytes in front of the first aligned dword and the up to eleven behind the last 12-byte group are
// stored byte by byte by up to fourteen lanes behind the others.  An output pixel is one source pixel (COPY), the mean of 2 x 2
// (HALF) or the two integer passes over 2 x 2 (LINEAR); a source pixel is one Y byte and, per chroma plane, one, two or four
// taps.  Frame payloads start at any byte of the chunk ("FRAME\n" is six bytes), so every load is a byte load: neighbouring
// lanes read neighbouring bytes of the same lines and the planes are read once from memory, the repeats come from L1 / L2.
// Kernels index by thread only: no LDS, no barrier, no cross-lane operation, plain C++ and vector memory operations.
#include "common.h"

namespace pr {
namespace {

constexpr int kYuvThreads = 256;
constexpr int kYuvLaneBytes = 12;
constexpr int kYuvEndLanes = 3 + kYuvLaneBytes - 1;   // byte lanes: the head and what is left behind the last group
enum { kAxisFull = 0, kAxisCentred = 1, kAxisCosited = 2 };

struct YuvParams {
  const uint8_t* data;
  const int64_t* offsets;
  uint8_t* dst;
  const int32_t* xofs;
  const int16_t* xcoef;
  const int32_t* yofs;
  const int16_t* ycoef;
  long data_bytes;
  int cy, crv, cbu, cgu, cgv, yo;
  int H, W, h, w;
  int cw, ch;            // the chroma planes' size
  int xkind, ykind;      // kAxis* of the chroma planes
  int mono, bgr;
  int frame_bytes;       // one source frame's payload
  int pixels;            // h * w
  int head;              // bytes in front of the first aligned dword of dst: 0..3 (the whole call when it is shorter)
  long total;            // F * h * w * 3
  long groups;           // 12-byte groups of aligned dwords
};

struct Taps {
  int i0, i1, w0, w1;    // w0 + w1 = 4
};

// The two taps of full-resolution sample `pos` of an axis whose plane has `size` samples.
__device__ __forceinline__ Taps chroma_taps(int kind, int pos, int size) {
  if (kind == kAxisFull) return Taps{pos, pos, 4, 0};
  const int i = pos >> 1;
  if (pos & 1) {
    const int j = min(i + 1, size - 1);
    return kind == kAxisCentred ? Taps{i, j, 3, 1} : Taps{i, j, 2, 2};
  }
  return kind == kAxisCentred ? Taps{i, max(i - 1, 0), 3, 1} : Taps{i, i, 4, 0};
}

// C16 of one chroma plane: the product of the two axes' taps, weights summing to 16.
__device__ __forceinline__ int chroma16(const uint8_t* plane, int cw, const Taps& tx, const Taps& ty) {
  const uint8_t* r0 = plane + ty.i0 * cw;
  int s = ty.w0 * (tx.w0 * r0[tx.i0] + (tx.w1 ? tx.w1 * r0[tx.i1] : 0));
  if (ty.w1) {
    const uint8_t* r1 = plane + ty.i1 * cw;
    s += ty.w1 * (tx.w0 * r1[tx.i0] + (tx.w1 ? tx.w1 * r1[tx.i1] : 0));
  }
  return s;
}

__device__ __forceinline__ unsigned clamp8(int v) { return (unsigned)min(max(v, 0), 255); }

// Source pixel (Y, X) of the frame whose payload starts at `base`, as its three output bytes (the first in bits 0..7).
__device__ __forceinline__ unsigned yuv_pixel(const YuvParams& p, const uint8_t* base, int Y, int X) {
  if (!base) return 0;                                // a payload outside the chunk: zeros, nothing read
  const int y = 16 * ((int)base[Y * p.W + X] - p.yo);
  int u = 0, v = 0;
  if (!p.mono) {
    const Taps tx = chroma_taps(p.xkind, X, p.cw), ty = chroma_taps(p.ykind, Y, p.ch);
    const uint8_t* up = base + p.H * p.W;
    u = chroma16(up, p.cw, tx, ty) - 2048;
    v = chroma16(up + p.cw * p.ch, p.cw, tx, ty) - 2048;
  }
  const int luma = p.cy * y + (1 << 19);
  const unsigned r = clamp8((luma + p.crv * v) >> 20);
  const unsigned g = clamp8((luma - p.cgu * u - p.cgv * v) >> 20);
  const unsigned b = clamp8((luma + p.cbu * u) >> 20);
  return p.bgr ? (b | g << 8 | r << 16) : (r | g << 8 | b << 16);
}

// Output pixel (y, x) of that frame: j3's three modes over yuv_pixel.
template <int MODE>
__device__ __forceinline__ unsigned out_pixel(const YuvParams& p, const uint8_t* base, int y, int x) {
  if (MODE == PR_RESIZE_COPY) return yuv_pixel(p, base, y, x);
  if (MODE == PR_RESIZE_HALF) {
    const unsigned a = yuv_pixel(p, base, 2 * y, 2 * x), b = yuv_pixel(p, base, 2 * y, 2 * x + 1);
    const unsigned c = yuv_pixel(p, base, 2 * y + 1, 2 * x), d = yuv_pixel(p, base, 2 * y + 1, 2 * x + 1);
    unsigned o = 0;
#pragma unroll
    for (int k = 0; k < 24; k += 8) o |= ((((a >> k) & 255) + ((b >> k) & 255) + ((c >> k) & 255) + ((d >> k) & 255) + 2) >> 2) << k;
    return o;
  }
  // the plan's offsets lie in 0..S-1; clamped all the same, so that no table content can form an address outside the frame
  const int x0 = min(max(p.xofs[x], 0), p.W - 1), x1 = min(x0 + 1, p.W - 1);
  const int y0 = min(max(p.yofs[y], 0), p.H - 1), y1 = min(y0 + 1, p.H - 1);
  const int a0 = p.xcoef[2 * x], a1 = p.xcoef[2 * x + 1], b0 = p.ycoef[2 * y], b1 = p.ycoef[2 * y + 1];
  const unsigned s00 = yuv_pixel(p, base, y0, x0), s01 = yuv_pixel(p, base, y0, x1);
  const unsigned s10 = yuv_pixel(p, base, y1, x0), s11 = yuv_pixel(p, base, y1, x1);
  unsigned o = 0;
#pragma unroll
  for (int k = 0; k < 24; k += 8) {
    const int t0 = (int)((s00 >> k) & 255) * a0 + (int)((s01 >> k) & 255) * a1;
    const int t1 = (int)((s10 >> k) & 255) * a0 + (int)((s11 >> k) & 255) * a1;
    o |= (unsigned)((((b0 * (t0 >> 4)) >> 16) + ((b1 * (t1 >> 4)) >> 16) + 2) >> 2) << k;
  }
  return o;
}

// Frame f's payload, or null where its offset does not leave the whole payload inside the chunk.
__device__ __forceinline__ const uint8_t* frame_base(const YuvParams& p, long f) {
  const long off = p.offsets[f];
  return (off >= 0 && off <= p.data_bytes - p.frame_bytes) ? p.data + off : nullptr;
}

template <int MODE>
__global__ void __launch_bounds__(kYuvThreads) yuv_frames_kernel(YuvParams p) {
  const long g = (long)blockIdx.x * kYuvThreads + threadIdx.x;
  int count = kYuvLaneBytes;
  long n;                                             // the lane's first byte in the flat output
  if (g < p.groups) {
    n = p.head + (long)kYuvLaneBytes * g;
  } else {                                            // the unaligned ends: one byte a lane
    const long e = g - p.groups;
    const long tail0 = p.head + (long)kYuvLaneBytes * p.groups;
    n = e < p.head ? e : tail0 + (e - p.head);
    if (n >= p.total) return;
    count = 1;
  }
  const long q = n / 3;                               // the lane's first output pixel, counted through the whole call
  const int skip = (int)(n - 3 * q);                  // bytes of that pixel in front of the lane's first
  const int np = (skip + count + 2) / 3;              // pixels the lane touches: 1 (a byte lane), 4 or 5
  long f = q / p.pixels;
  const int rem = (int)(q - f * p.pixels);
  int y = rem / p.w, x = rem - y * p.w;
  const uint8_t* base = frame_base(p, f);
  unsigned __int128 run = 0;
  for (int i = 0; i < np; ++i) {
    if (i && ++x == p.w) {
      x = 0;
      if (++y == p.h) y = 0, base = frame_base(p, ++f);
    }
    run |= (unsigned __int128)out_pixel<MODE>(p, base, y, x) << (24 * i);
  }
  run >>= 8 * skip;
  if (count == 1) {
    p.dst[n] = (uint8_t)run;
    return;
  }
  const unsigned words[3] = {(unsigned)run, (unsigned)(run >> 32), (unsigned)(run >> 64)};
  __builtin_memcpy(__builtin_assume_aligned(p.dst + n, 4), words, sizeof words);
}

}  // namespace
}  // namespace pr

extern "C" int pr_yuv_frames(const pr_yuv_args* a, void* stream) {
  using namespace pr;
  PR_REQUIRE(a, "pr_yuv_frames: null args");
  PR_REQUIRE(a->F >= 0, "pr_yuv_frames: F = %d", a->F);
  if (a->F == 0) return PR_OK;
  PR_REQUIRE(a->H >= 1 && a->H <= PR_RESIZE_MAX_SIDE && a->W >= 1 && a->W <= PR_RESIZE_MAX_SIDE,
             "pr_yuv_frames: %d x %d frames: every side must lie in 1..%d", a->W, a->H, PR_RESIZE_MAX_SIDE);
  PR_REQUIRE(a->chroma >= PR_Y4M_C420JPEG && a->chroma <= PR_Y4M_CMONO, "pr_yuv_frames: chroma = %d (PR_Y4M_C420JPEG .. PR_Y4M_CMONO)",
             a->chroma);
  PR_REQUIRE(a->data_bytes >= 0, "pr_yuv_frames: data_bytes = %lld", (long long)a->data_bytes);
  PR_REQUIRE(a->data, "pr_yuv_frames: null data");
  PR_REQUIRE(a->offsets, "pr_yuv_frames: null offsets");
  PR_REQUIRE(a->dst, "pr_yuv_frames: null dst");
  const bool scaled = a->h || a->w || a->mode || a->xofs || a->xcoef || a->yofs || a->ycoef;
  int h = a->H, w = a->W, mode = PR_RESIZE_COPY;
  if (scaled) {
    h = a->h, w = a->w, mode = a->mode;
    PR_REQUIRE(h >= 1 && h <= PR_RESIZE_MAX_SIDE && w >= 1 && w <= PR_RESIZE_MAX_SIDE,
               "pr_yuv_frames: %d x %d -> %d x %d: every side must lie in 1..%d (h = w = 0, mode 0 and no tables: no downscale)", a->W,
               a->H, w, h, PR_RESIZE_MAX_SIDE);
    const int want = (a->H == h && a->W == w) ? PR_RESIZE_COPY : (a->W == 2 * w && a->H == 2 * h) ? PR_RESIZE_HALF : PR_RESIZE_LINEAR;
    PR_REQUIRE(mode == want, "pr_yuv_frames: mode = %d, but %d x %d -> %d x %d is mode %d (pass what pr_resize_plan gave)", mode, a->W,
               a->H, w, h, want);
    PR_REQUIRE(a->xofs, "pr_yuv_frames: null xofs");
    PR_REQUIRE(a->xcoef, "pr_yuv_frames: null xcoef");
    PR_REQUIRE(a->yofs, "pr_yuv_frames: null yofs");
    PR_REQUIRE(a->ycoef, "pr_yuv_frames: null ycoef");
  }
  YuvParams p;
  p.data = a->data, p.offsets = a->offsets, p.dst = a->dst;
  p.xofs = a->xofs, p.xcoef = a->xcoef, p.yofs = a->yofs, p.ycoef = a->ycoef;
  p.data_bytes = (long)a->data_bytes;
  p.cy = a->plan.cy, p.crv = a->plan.crv, p.cbu = a->plan.cbu, p.cgu = a->plan.cgu, p.cgv = a->plan.cgv, p.yo = a->plan.yo;
  p.H = a->H, p.W = a->W, p.h = h, p.w = w;
  const bool half_w = a->chroma == PR_Y4M_C420JPEG || a->chroma == PR_Y4M_C420MPEG2 || a->chroma == PR_Y4M_C422;
  const bool half_h = a->chroma == PR_Y4M_C420JPEG || a->chroma == PR_Y4M_C420MPEG2;
  p.mono = a->chroma == PR_Y4M_CMONO;
  p.cw = half_w ? (a->W + 1) / 2 : a->W;
  p.ch = half_h ? (a->H + 1) / 2 : a->H;
  p.xkind = !half_w ? kAxisFull : a->chroma == PR_Y4M_C420JPEG ? kAxisCentred : kAxisCosited;
  p.ykind = half_h ? kAxisCentred : kAxisFull;
  p.bgr = a->bgr != 0;
  p.frame_bytes = a->H * a->W + (p.mono ? 0 : 2 * p.cw * p.ch);
  p.pixels = h * w;
  p.total = (long)a->F * p.pixels * 3;
  p.head = (int)std::min<long>((long)(-(uintptr_t)a->dst & 3), p.total);
  p.groups = (p.total - p.head) / kYuvLaneBytes;
  const long lanes = p.groups + kYuvEndLanes;
  const long blocks = ceil_div(lanes, (long)kYuvThreads);
  PR_REQUIRE(blocks <= 0x7fffffffl, "pr_yuv_frames: %d frames of %d x %d are too many bytes for one call", a->F, w, h);
  const dim3 grid((unsigned)blocks), block(kYuvThreads);
  if (mode == PR_RESIZE_COPY) {
    hipLaunchKernelGGL(yuv_frames_kernel<PR_RESIZE_COPY>, grid, block, 0, (hipStream_t)stream, p);
  } else if (mode == PR_RESIZE_HALF) {
    hipLaunchKernelGGL(yuv_frames_kernel<PR_RESIZE_HALF>, grid, block, 0, (hipStream_t)stream, p);
  } else {
    hipLaunchKernelGGL(yuv_frames_kernel<PR_RESIZE_LINEAR>, grid, block, 0, (hipStream_t)stream, p);
  }
  return check_launch("yuv_frames_kernel");
}
