// The person detector's bf16 convolution (include/poserisk_hip.h, section j8, paragraph "bf16"): implicit GEMM on
// v_mfma_f32_32x32x16_bf16, NHWC,
//   y[m][n] = round(act(sum_k W[n][k] * X[m][k] + b[n]) [+ (float)res[m][n]])      m = (image, ho, wo), k = (kh, kw, ci)
// with bf16 operands, fp32 accumulation and ONE rounding at the store (none for fp32 output: the heads), for 3x3 and 1x1
// kernels of stride 1 and 2, padding k / 2, any Cin % 8 == 0 and any Cout.
//
// One workgroup of four waves computes 128 pixels x 64 channels; wave w owns pixels 32 w .. 32 w + 31 and all 64 channels as
// two 32 x 32 accumulators, the WEIGHTS as the MFMA's A operand and the pixels as B (det_conv.hip's orientation: a lane's
// sixteen accumulators are four runs of four consecutive channels of one pixel).  K is walked in stages of 64 bf16 (128
// bytes a row) through ONE LDS buffer: stage kt + 1 is fetched into registers while stage kt is multiplied, and written
// between two barriers.  (Two buffers and one barrier a stage were measured first: 55 KB of LDS held a CU to two workgroups
// and the network ran 1.2x slower; with 34 KB four fit, and other workgroups' MFMAs fill this one's barrier gaps.)
// Rows are 144 bytes apart: 16-byte aligned, and 9 slots of 16
// bytes is odd, so the sixteen rows of one ds_read_b128 lane group ({0-3, 12-15, 20-27} and its three siblings: sixteen
// distinct rows modulo 16) fall into sixteen distinct slots of the 256-byte bank row.  The epilogue goes through LDS as
// well: the activated fp32 tile is laid down as [128][64] (rows 272 bytes apart) and picked up with a thread on 8
// consecutive channels of a pixel, so the residual comes in and the result leaves 16 bytes a lane and 128 contiguous bytes
// an eight-lane run, instead of 8-byte runs 2 * Cout apart.  Where Cout % 8 != 0, or the output is fp32, a lane takes one
// value with consecutive lanes on consecutive channels (2- or 4-byte accesses).
// Every global access goes through a raw buffer descriptor of the tensor's own size: a padding-ring tap, a row past the
// ragged last tile, a k past K and a channel past Cout get the out-of-range offset, read zeros and store nothing.  No
// workgroup talks to another and the k order is fixed: a frame's bits do not depend on its batch.
#include "det_conv.h"
#include "kernel_vocab.h"

namespace pr {
namespace {

constexpr int kBM = 128, kBN = 64, kBK = 64, kThreads = 256;
constexpr int kPitch = 2 * kBK + 16;                   // bytes between the LDS rows of a stage
constexpr int kStageBytes = (kBM + kBN) * kPitch;      // weights rows first, then the pixels'
constexpr int kEpiPitch = kBN + 4;                     // floats between the rows of the epilogue's tile
constexpr int kEpiBytes = kBM * kEpiPitch * 4;
[[maybe_unused]] constexpr int kLdsBytes = kEpiBytes > kStageBytes ? kEpiBytes : kStageBytes;      // the epilogue's tile reuses the stage's bytes

template <typename Rsrc>
__device__ __forceinline__ u32x4 load16(Rsrc rsrc, unsigned voffset) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_raw_buffer_load_b128(rsrc, voffset, 0, 0);
#else
  return u32x4{0u, 0u, 0u, 0u};
#endif
}

__device__ __forceinline__ float bf16_lo(unsigned w) { return __builtin_bit_cast(float, w << 16); }
__device__ __forceinline__ float bf16_hi(unsigned w) { return __builtin_bit_cast(float, w & 0xffff0000u); }

// leaky(acc + b): each operation rounded on its own, as the header states it
#pragma clang fp contract(off)
__device__ __forceinline__ float det_act(float acc, float b, int leaky) {
  const float v = acc + b;
  return (leaky && !(v > 0.f)) ? 0.1f * v : v;
}

__global__ void __launch_bounds__(kThreads) det_conv_bf16_kernel(DetConvBf16Problem p) {
#if defined(__HIP_DEVICE_COMPILE__)
  __shared__ __attribute__((aligned(16))) unsigned char smem[kLdsBytes];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int M = p.B * p.Ho * p.Wo;
  const int K = p.ksize * p.ksize * p.Cin;
  const int m0 = blockIdx.x * kBM, n0 = blockIdx.y * kBN;
  const int pad = p.ksize >> 1;
  const auto xsrc = make_rsrc(p.x, p.B * p.H * p.W * p.Cin * 2);
  const auto wsrc = make_rsrc(p.w, p.cout_pad * p.kpad * 2);

  // loader: thread -> rows (tid >> 3) + 32 i of both operands, 16-byte chunk tid & 7 (8 bf16) of the stage's 64 k.  Cin % 8 == 0:
  // a chunk never straddles a tap.
  const int chunk = tid & 7, row = tid >> 3;
  int pbase[4], hi0[4], wi0[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int m = m0 + row + 32 * i;
    if (m < M) {
      const int b = m / (p.Ho * p.Wo), r = m - b * (p.Ho * p.Wo);
      const int ho = r / p.Wo, wo = r - ho * p.Wo;
      pbase[i] = b * p.H * p.W, hi0[i] = ho * p.stride - pad, wi0[i] = wo * p.stride - pad;
    } else {
      pbase[i] = 0, hi0[i] = -0x10000, wi0[i] = -0x10000;     // every tap of it is outside the map
    }
  }
  u32x4 gx[4], gw[2];
  auto fetch = [&](int kt) {
    const int k = kt * kBK + 8 * chunk;
    const int tap = k / p.Cin, ci = k - tap * p.Cin;
    const int kh = tap / p.ksize, kw = tap - kh * p.ksize;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int hi = hi0[i] + kh, wi = wi0[i] + kw;
      const bool in = k < K && hi >= 0 && hi < p.H && wi >= 0 && wi < p.W;
      gx[i] = load16(xsrc, in ? (unsigned)(((pbase[i] + hi * p.W + wi) * p.Cin + ci) * 2) : kOOB);
    }
#pragma unroll
    for (int i = 0; i < 2; ++i)      // kpad is a multiple of 32, a stage of 64: the last one may end half way along the row
      gw[i] = load16(wsrc, k < p.kpad ? (unsigned)(((n0 + row + 32 * i) * p.kpad + k) * 2) : kOOB);
  };
  auto stage = [&]() {
    unsigned char* s = smem + row * kPitch + 16 * chunk;
#pragma unroll
    for (int i = 0; i < 2; ++i) *reinterpret_cast<u32x4*>(s + 32 * i * kPitch) = gw[i];
#pragma unroll
    for (int i = 0; i < 4; ++i) *reinterpret_cast<u32x4*>(s + (kBN + 32 * i) * kPitch) = gx[i];
  };

  f32x16 acc[2];
#pragma unroll
  for (int nt = 0; nt < 2; ++nt)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[nt][e] = 0.f;
  // fragment: lane (r = lane & 31, half = lane >> 5) supplies k = 8 half .. 8 half + 7 of an MFMA's 16: chunk 2 s + half of its
  // row in step s, the same k for both operands
  const int r = lane & 31, half = lane >> 5;
  const int fw = r * kPitch + 16 * half, fx = (kBN + 32 * wave + r) * kPitch + 16 * half;
  const int nk = (p.kpad + kBK - 1) / kBK;
  fetch(0);
  for (int kt = 0; kt < nk; ++kt) {
    stage();
    __syncthreads();
    if (kt + 1 < nk) fetch(kt + 1);
    const unsigned char* s = smem;
#pragma unroll
    for (int st = 0; st < 4; ++st) {
      const bf16x8 b = *reinterpret_cast<const bf16x8*>(s + fx + 32 * st);
      const bf16x8 a0 = *reinterpret_cast<const bf16x8*>(s + fw + 32 * st);
      const bf16x8 a1 = *reinterpret_cast<const bf16x8*>(s + fw + 32 * kPitch + 32 * st);
      acc[0] = mfma_bf16_step(a0, b, acc[0]);
      acc[1] = mfma_bf16_step(a1, b, acc[1]);
    }
    __syncthreads();
  }

  // epilogue.  acc[nt][4 q + j] = channel n0 + 32 nt + 8 q + 4 half + j of pixel m0 + 32 wave + r: activated, laid down as fp32
  float* epi = reinterpret_cast<float*>(smem);
#pragma unroll
  for (int nt = 0; nt < 2; ++nt)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int c = 32 * nt + 8 * q + 4 * half;
      const f32x4 b = *reinterpret_cast<const f32x4*>(p.bias + n0 + c);      // the bias is padded to the tile
      f32x4 v;
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = det_act(acc[nt][4 * q + j], b[j], p.leaky);
      *reinterpret_cast<f32x4*>(epi + (32 * wave + r) * kEpiPitch + c) = v;
    }
  __syncthreads();
  const int esize = p.out_f32 ? 4 : 2;
  const auto ysrc = make_rsrc(p.y, M * p.Cout * esize);
  const auto rsrc = make_rsrc(p.res ? p.res : p.y, M * p.Cout * 2);
  if (!p.out_f32 && (p.Cout & 7) == 0) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int pr = row + 32 * i, pix = m0 + pr, c = n0 + 8 * chunk;
      const unsigned off = (pix < M && c < p.Cout) ? ((unsigned)pix * (unsigned)p.Cout + (unsigned)c) * 2u : kOOB;
      const f32x4 v0 = *reinterpret_cast<const f32x4*>(epi + pr * kEpiPitch + 8 * chunk);
      const f32x4 v1 = *reinterpret_cast<const f32x4*>(epi + pr * kEpiPitch + 8 * chunk + 4);
      float v[8] = {v0[0], v0[1], v0[2], v0[3], v1[0], v1[1], v1[2], v1[3]};
      if (p.res) {
        const u32x4 rr = load16(rsrc, off);
#pragma unroll
        for (int j = 0; j < 4; ++j) v[2 * j] = v[2 * j] + bf16_lo(rr[j]), v[2 * j + 1] = v[2 * j + 1] + bf16_hi(rr[j]);
      }
      const u32x4 o = {pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3]), pack_bf16x2(v[4], v[5]), pack_bf16x2(v[6], v[7])};
      buffer_store_b128_sreg(o, ysrc, off, 0);
    }
  } else {
    for (int e = tid; e < kBM * kBN; e += kThreads) {
      const int pr = e >> 6, ch = e & 63, pix = m0 + pr, c = n0 + ch;
      const bool ok = pix < M && c < p.Cout;
      const unsigned idx = (unsigned)pix * (unsigned)p.Cout + (unsigned)c;
      float v = epi[pr * kEpiPitch + ch];
      if (p.res) v = v + bf16_lo((unsigned)__builtin_amdgcn_raw_buffer_load_b16(rsrc, ok ? idx * 2u : kOOB, 0, 0));
      if (p.out_f32) __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), ysrc, ok ? idx * 4u : kOOB, 0, 0);
      else __builtin_amdgcn_raw_buffer_store_b16((unsigned short)(pack_bf16x2(v, 0.f) & 0xffffu), ysrc, ok ? idx * 2u : kOOB, 0, 0);
    }
  }
#endif
}

}  // namespace

int det_conv_bf16_launch(const DetConvBf16Problem& p, hipStream_t stream) {
  PR_REQUIRE(p.x && p.w && p.bias && p.y, "det_conv_bf16: null tensor");
  PR_REQUIRE(p.ksize == 1 || p.ksize == 3, "det_conv_bf16: ksize = %d, must be 1 or 3", p.ksize);
  PR_REQUIRE(p.stride == 1 || p.stride == 2, "det_conv_bf16: stride = %d, must be 1 or 2", p.stride);
  PR_REQUIRE(p.B >= 1 && p.H >= 1 && p.W >= 1 && p.Cin >= 8 && p.Cin % 8 == 0 && p.Cout >= 1,
             "det_conv_bf16: B %d, H %d, W %d, Cin %d (a multiple of 8), Cout %d", p.B, p.H, p.W, p.Cin, p.Cout);
  const int pad = p.ksize / 2;
  PR_REQUIRE(p.Ho == (p.H + 2 * pad - p.ksize) / p.stride + 1 && p.Wo == (p.W + 2 * pad - p.ksize) / p.stride + 1,
             "det_conv_bf16: output %d x %d does not belong to input %d x %d, kernel %d, stride %d", p.Wo, p.Ho, p.W, p.H, p.ksize,
             p.stride);
  PR_REQUIRE(p.cout_pad % kBN == 0 && p.cout_pad >= p.Cout && p.cout_pad - p.Cout < kBN, "det_conv_bf16: cout_pad = %d for Cout = %d",
             p.cout_pad, p.Cout);
  PR_REQUIRE(p.kpad % 32 == 0 && p.kpad >= p.ksize * p.ksize * p.Cin && p.kpad - p.ksize * p.ksize * p.Cin < 32,
             "det_conv_bf16: kpad = %d for K = %d", p.kpad, p.ksize * p.ksize * p.Cin);
  PR_REQUIRE(((uintptr_t)p.x | (uintptr_t)p.w | (uintptr_t)p.bias | (uintptr_t)p.y | (uintptr_t)p.res) % 16 == 0,
             "det_conv_bf16: a tensor is not 16-byte aligned");
  const long lim = 0x7fffffffl;
  PR_REQUIRE((long)p.B * p.H * p.W * p.Cin * 2 <= lim && p.M() * p.Cout * 4 <= lim && (long)p.cout_pad * p.kpad * 2 <= lim,
             "det_conv_bf16: a tensor of 2 GiB or more (B %d, %d x %d x %d -> %d x %d x %d)", p.B, p.H, p.W, p.Cin, p.Ho, p.Wo, p.Cout);
  const dim3 grid((unsigned)ceil_div(p.M(), (long)kBM), (unsigned)(p.cout_pad / kBN));
  hipLaunchKernelGGL(det_conv_bf16_kernel, grid, dim3(kThreads), 0, stream, p);
  return check_launch("det_conv_bf16_kernel");
}

}  // namespace pr
