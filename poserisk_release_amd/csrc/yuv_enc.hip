// Device half of the YUV4MPEG2 writer: u8[F,H,W,3] -> the bytes of F frames of a stream ("FRAME\n", the Y plane, the U plane,
// the V plane, frame after frame without padding) by the contract of include/poserisk_hip.h (section j7): edge-replicating
// padding to out_W x out_H, the integer forward matrix, chroma subsampling with one rounding a sample.
// tests/yuv_enc_ref.py restates the contract in numpy, tests/test_y4m_write_native.py runs this file on the host under
// sanitizers, tests/test_y4m_write_gpu.py on the device.
//
// As in yuv.hip and resize.hip the output of a call is one flat run written in ALIGNED DWORDS, one a lane: a wave stores 256
// consecutive bytes.  A frame is 6 + frame_bytes bytes, so plane and frame boundaries fall at any byte of a dword: a lane finds
// the place of its first byte in the stream once (frame, byte in the frame, row and column in the plane) and walks on from
// there byte by byte, so a dword may hold the tail of V, a FRAME header and the next frame's first Y samples.  The up to three
// bytes in front of the first aligned dword and the up to three behind the last are stored byte by byte by up to six lanes
// behind the others.  A sample's taps are read from src where the sample is made, each pixel's three bytes once: within a
// plane row neighbouring lanes read neighbouring pixels of the same source lines, the taps two neighbouring samples share
// come from L1.  Kernels index by thread only: no LDS, no barrier, no cross-lane operation, plain C++ and vector memory
// operations.
#include "common.h"

namespace pr {
namespace {

constexpr int kEncThreads = 256;
constexpr int kEncEndLanes = 6;        // byte lanes: up to three in front of the first aligned dword, three behind the last
constexpr int kFrameHeader = 6;        // "FRAME\n"

struct EncParams {
  const uint8_t* src;
  uint8_t* dst;
  pr_yuv_enc_coeffs k;
  int H, W, oH, oW;
  int cw, ch;              // the chroma planes' size (0, 0 for mono)
  int chroma, bgr;
  int luma_bytes;          // oH * oW
  int plane_bytes;         // cw * ch
  int frame_size;          // 6 + luma_bytes + 2 * plane_bytes
  int head;                // bytes in front of the first aligned dword of dst: 0..3 (the whole call when it is shorter)
  long total;              // F * frame_size
  long words;              // aligned dwords
};

struct Rgb {
  int r, g, b;
};

// Pixel (y, x) of the padded picture: indices outside the source take the nearest source pixel.
__device__ __forceinline__ Rgb pixel(const EncParams& p, const uint8_t* frame, int y, int x) {
  const uint8_t* q = frame + ((long)min(max(y, 0), p.H - 1) * p.W + min(max(x, 0), p.W - 1)) * 3;
  const int c0 = q[0], c1 = q[1], c2 = q[2];
  return p.bgr ? Rgb{c2, c1, c0} : Rgb{c0, c1, c2};
}

__device__ __forceinline__ void add(Rgb& s, const Rgb& a, int w) { s.r += w * a.r, s.g += w * a.g, s.b += w * a.b; }

__device__ __forceinline__ unsigned clamp8(int v) { return (unsigned)min(max(v, 0), 255); }

// Luma sample (y, x) of the frame at `frame`.
__device__ __forceinline__ unsigned luma(const EncParams& p, const uint8_t* frame, int y, int x) {
  const Rgb c = pixel(p, frame, y, x);
  return (unsigned)(p.k.yo + ((p.k.kyr * c.r + p.k.kyg * c.g + p.k.kyb * c.b + (1 << 15)) >> 16));
}

// Chroma sample (j, i) of plane `v` (0: U, 1: V): the layout's tap sums, then the matrix row with the taps' weight in the shift.
__device__ __forceinline__ unsigned chroma_sample(const EncParams& p, const uint8_t* frame, int v, int j, int i) {
  Rgb s{0, 0, 0};
  int log_t = 0;
  if (p.chroma == PR_Y4M_C444) {
    s = pixel(p, frame, j, i);
  } else if (p.chroma == PR_Y4M_C420JPEG) {
    log_t = 2;
    add(s, pixel(p, frame, 2 * j, 2 * i), 1), add(s, pixel(p, frame, 2 * j, 2 * i + 1), 1);
    add(s, pixel(p, frame, 2 * j + 1, 2 * i), 1), add(s, pixel(p, frame, 2 * j + 1, 2 * i + 1), 1);
  } else {                                             // 422 and 420mpeg2: co-sited columns, weights 1 2 1
    const int rows = p.chroma == PR_Y4M_C420MPEG2 ? 2 : 1;
    const int y0 = rows == 2 ? 2 * j : j;
    log_t = rows == 2 ? 3 : 2;
    for (int r = 0; r < rows; ++r) {
      add(s, pixel(p, frame, y0 + r, 2 * i - 1), 1), add(s, pixel(p, frame, y0 + r, 2 * i), 2);
      add(s, pixel(p, frame, y0 + r, 2 * i + 1), 1);
    }
  }
  const int half = 1 << (15 + log_t);
  const int sum = v ? p.k.kc * s.r - p.k.kvg * s.g - p.k.kvb * s.b : p.k.kc * s.b - p.k.kur * s.r - p.k.kug * s.g;
  return clamp8(128 + ((sum + half) >> (16 + log_t)));
}

// A place in the stream: byte r of frame f, which is byte (row, col) of the plane it lies in (nothing for the FRAME header).
struct Place {
  long f;
  int r, row, col;
};

__device__ __forceinline__ Place place_of(const EncParams& p, long n) {
  Place a;
  a.f = n / p.frame_size;
  a.r = (int)(n - a.f * p.frame_size);
  a.row = a.col = 0;
  int q = a.r - kFrameHeader;
  if (q >= 0) {
    int width = p.oW;
    if (q >= p.luma_bytes) {
      q -= p.luma_bytes;
      if (q >= p.plane_bytes) q -= p.plane_bytes;
      width = p.cw;
    }
    a.row = q / width, a.col = q - a.row * width;
  }
  return a;
}

__device__ __forceinline__ void advance(const EncParams& p, Place& a) {
  if (++a.r == p.frame_size) a.r = 0, ++a.f;
  const int q = a.r - kFrameHeader;
  if (q <= 0 || q == p.luma_bytes || q == p.luma_bytes + p.plane_bytes) {    // a header byte, or a plane's first
    a.row = a.col = 0;
  } else if (++a.col == (q < p.luma_bytes ? p.oW : p.cw)) {
    a.col = 0, ++a.row;
  }
}

__device__ __forceinline__ unsigned stream_byte(const EncParams& p, const Place& a) {
  if (a.r < kFrameHeader) return (unsigned)"FRAME\n"[a.r];
  const uint8_t* frame = p.src + a.f * ((long)p.H * p.W * 3);
  const int q = a.r - kFrameHeader;
  if (q < p.luma_bytes) return luma(p, frame, a.row, a.col);
  return chroma_sample(p, frame, q - p.luma_bytes >= p.plane_bytes, a.row, a.col);
}

__global__ void __launch_bounds__(kEncThreads) yuv_encode_kernel(EncParams p) {
  const long g = (long)blockIdx.x * kEncThreads + threadIdx.x;
  if (g >= p.words) {                                 // the unaligned ends: one byte a lane
    const long e = g - p.words;
    const long tail0 = p.head + 4 * p.words;
    const long n = e < p.head ? e : tail0 + (e - p.head);
    if (n >= p.total) return;
    p.dst[n] = (uint8_t)stream_byte(p, place_of(p, n));
    return;
  }
  const long n = p.head + 4 * g;
  Place a = place_of(p, n);
  unsigned word = stream_byte(p, a);
#pragma unroll
  for (int i = 1; i < 4; ++i) {
    advance(p, a);
    word |= stream_byte(p, a) << (8 * i);
  }
  __builtin_memcpy(__builtin_assume_aligned(p.dst + n, 4), &word, sizeof word);
}

}  // namespace
}  // namespace pr

extern "C" int pr_yuv_encode(const pr_yuv_enc_args* a, void* stream) {
  using namespace pr;
  PR_REQUIRE(a, "pr_yuv_encode: null args");
  PR_REQUIRE(a->F >= 0, "pr_yuv_encode: F = %d", a->F);
  if (a->F == 0) return PR_OK;
  PR_REQUIRE(a->H >= 1 && a->H <= PR_RESIZE_MAX_SIDE && a->W >= 1 && a->W <= PR_RESIZE_MAX_SIDE,
             "pr_yuv_encode: %d x %d frames: every side must lie in 1..%d", a->W, a->H, PR_RESIZE_MAX_SIDE);
  PR_REQUIRE(a->out_H - a->H >= 0 && a->out_H - a->H <= 1 && a->out_W - a->W >= 0 && a->out_W - a->W <= 1,
             "pr_yuv_encode: %d x %d frames padded to %d x %d: a side grows by 0 or 1", a->W, a->H, a->out_W, a->out_H);
  PR_REQUIRE(a->out_H <= PR_RESIZE_MAX_SIDE && a->out_W <= PR_RESIZE_MAX_SIDE,
             "pr_yuv_encode: the padded picture %d x %d: every side must lie in 1..%d", a->out_W, a->out_H, PR_RESIZE_MAX_SIDE);
  PR_REQUIRE(a->chroma >= PR_Y4M_C420JPEG && a->chroma <= PR_Y4M_CMONO, "pr_yuv_encode: chroma = %d (PR_Y4M_C420JPEG .. PR_Y4M_CMONO)",
             a->chroma);
  PR_REQUIRE(a->src, "pr_yuv_encode: null src");
  PR_REQUIRE(a->dst, "pr_yuv_encode: null dst");
  EncParams p;
  p.src = a->src, p.dst = a->dst, p.k = a->plan;
  p.H = a->H, p.W = a->W, p.oH = a->out_H, p.oW = a->out_W;
  const bool half_w = a->chroma == PR_Y4M_C420JPEG || a->chroma == PR_Y4M_C420MPEG2 || a->chroma == PR_Y4M_C422;
  const bool half_h = a->chroma == PR_Y4M_C420JPEG || a->chroma == PR_Y4M_C420MPEG2;
  const bool mono = a->chroma == PR_Y4M_CMONO;
  p.cw = mono ? 0 : half_w ? (p.oW + 1) / 2 : p.oW;
  p.ch = mono ? 0 : half_h ? (p.oH + 1) / 2 : p.oH;
  p.chroma = a->chroma, p.bgr = a->bgr != 0;
  p.luma_bytes = p.oH * p.oW;
  p.plane_bytes = p.cw * p.ch;
  p.frame_size = kFrameHeader + p.luma_bytes + 2 * p.plane_bytes;      // at most 6 + 3 * 4096^2
  p.total = (long)a->F * p.frame_size;
  p.head = (int)std::min<long>((long)(-(uintptr_t)a->dst & 3), p.total);
  p.words = (p.total - p.head) / 4;
  const long lanes = p.words + kEncEndLanes;
  const long blocks = ceil_div(lanes, (long)kEncThreads);
  PR_REQUIRE(blocks <= 0x7fffffffl, "pr_yuv_encode: %d frames of %d x %d are too many bytes for one call", a->F, p.oW, p.oH);
  hipLaunchKernelGGL(yuv_encode_kernel, dim3((unsigned)blocks), dim3(kEncThreads), 0, (hipStream_t)stream, p);
  return check_launch("yuv_encode_kernel");
}
