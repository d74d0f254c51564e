// The person detector's convolution (include/poserisk_hip.h, section j8): implicit GEMM on v_mfma_f32_32x32x2_f32, NHWC,
//   y[m][n] = act(sum_k W[n][k] * X[m][k] + b[n]) [+ res[m][n]]      m = (image, ho, wo), n = output channel, k = (kh, kw, ci)
// for 3x3 and 1x1 kernels of stride 1 and 2, padding k / 2, any Cin % 4 == 0 and any Cout (the packed weights and the bias are
// padded to the 64-channel tile, the stores are not).  A kernel of its own: the encoder's kernels, their plan and
// pr_conv2d_nhwc are untouched; only the vocabulary (kernel_vocab.h) is shared.
//
// One workgroup of four waves computes a tile of 64 pixels x 64 channels; wave (wm, wn) owns 32 x 32 of it with the WEIGHTS as
// the MFMA's A operand and the pixels as B, so that a lane's sixteen accumulators are four runs of four consecutive channels
// of ONE pixel: the epilogue loads the residual and stores the result 16 bytes at a time.  K is walked in stages of 32
// floats through LDS (rows of 36 floats: 16-byte aligned, and the sixteen rows a quarter wave reads lie in distinct banks);
// the next stage's global loads are in flight while the current one is multiplied.  Every global access goes through a raw
// buffer descriptor of the tensor's own size: a pixel of the padding ring, a row past the ragged last tile or a channel past
// Cout gets the out-of-range offset, reads zeros and stores nothing.  No cross-workgroup communication, one fixed k order:
// a frame's bits do not depend on its batch.
#include "det_conv.h"
#include "kernel_vocab.h"

namespace pr {
namespace {

constexpr int kBM = 64, kBN = 64, kBK = 32, kRow = 36, kThreads = 256;

__device__ __forceinline__ f32x4 load4(decltype(make_rsrc((float*)nullptr, 0)) rsrc, unsigned voffset) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsrc, voffset, 0, 0));
#else
  return f32x4{0.f, 0.f, 0.f, 0.f};
#endif
}

// leaky(acc + b) [+ res]: each operation rounded on its own, as the header states it
#pragma clang fp contract(off)
__device__ __forceinline__ float det_act(float acc, float b, int leaky) {
  const float v = acc + b;
  return (leaky && !(v > 0.f)) ? 0.1f * v : v;
}

// kOutBf16: y is bf16, each value rounded once when stored (layer 0 of a bf16 handle); false is the fp32 kernel, unchanged
template <bool kOutBf16>
__global__ void __launch_bounds__(kThreads) det_conv_kernel(DetConvProblem p) {
#if defined(__HIP_DEVICE_COMPILE__)
  __shared__ __attribute__((aligned(16))) float sW[kBN * kRow];
  __shared__ __attribute__((aligned(16))) float sX[kBM * kRow];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wn = wave & 1, wm = wave >> 1;
  const int M = p.B * p.Ho * p.Wo;
  const int K = p.ksize * p.ksize * p.Cin;
  const int m0 = blockIdx.x * kBM, n0 = blockIdx.y * kBN;
  const int pad = p.ksize >> 1;
  const auto xsrc = make_rsrc(p.x, p.B * p.H * p.W * p.Cin * 4);
  const auto wsrc = make_rsrc(p.w, p.cout_pad * p.kpad * 4);

  // loader: thread -> rows (tid >> 3) and (tid >> 3) + 32 of both operands, 16-byte chunk tid & 7 of the stage's 32 k
  const int chunk = tid & 7;
  int pbase[2], hi0[2], wi0[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int m = m0 + (tid >> 3) + 32 * i;
    if (m < M) {
      const int b = m / (p.Ho * p.Wo), r = m - b * (p.Ho * p.Wo);
      const int ho = r / p.Wo, wo = r - ho * p.Wo;
      pbase[i] = b * p.H * p.W, hi0[i] = ho * p.stride - pad, wi0[i] = wo * p.stride - pad;
    } else {
      pbase[i] = 0, hi0[i] = -0x10000, wi0[i] = -0x10000;     // every tap of it is outside the map
    }
  }
  f32x4 gx[2], gw[2];
  auto fetch = [&](int kt) {
    const int k = kt * kBK + 4 * chunk;
    const int tap = k / p.Cin, ci = k - tap * p.Cin;
    const int kh = tap / p.ksize, kw = tap - kh * p.ksize;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int hi = hi0[i] + kh, wi = wi0[i] + kw;
      const bool in = k < K && hi >= 0 && hi < p.H && wi >= 0 && wi < p.W;
      gx[i] = load4(xsrc, in ? (unsigned)(((pbase[i] + hi * p.W + wi) * p.Cin + ci) * 4) : kOOB);
      gw[i] = load4(wsrc, (unsigned)(((n0 + (tid >> 3) + 32 * i) * p.kpad + k) * 4));
    }
  };
  auto stage = [&]() {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int o = ((tid >> 3) + 32 * i) * kRow + 4 * chunk;
      *reinterpret_cast<f32x4*>(sX + o) = gx[i];
      *reinterpret_cast<f32x4*>(sW + o) = gw[i];
    }
  };

  f32x16 acc;
#pragma unroll
  for (int e = 0; e < 16; ++e) acc[e] = 0.f;
  // fragment: lane (row = lane & 31, half = lane >> 5) reads chunk 2 kk + half of its row: its four floats are the k of four
  // MFMAs, the same k for both operands
  const float* fW = sW + (wn * 32 + (lane & 31)) * kRow + 4 * (lane >> 5);
  const float* fX = sX + (wm * 32 + (lane & 31)) * kRow + 4 * (lane >> 5);
  const int nk = p.kpad / kBK;
  fetch(0);
  for (int kt = 0; kt < nk; ++kt) {
    stage();
    __syncthreads();
    if (kt + 1 < nk) fetch(kt + 1);
    f32x4 af[4], bf[4];
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      af[kk] = *reinterpret_cast<const f32x4*>(fW + 8 * kk);
      bf[kk] = *reinterpret_cast<const f32x4*>(fX + 8 * kk);
    }
#pragma unroll
    for (int kk = 0; kk < 4; ++kk)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(af[kk][j], bf[kk][j], acc, 0, 0, 0);
    __syncthreads();
  }

  // epilogue: acc[4 q + j] = channel n0 + 32 wn + 8 q + 4 (lane >> 5) + j of pixel m0 + 32 wm + (lane & 31)
  const int pix = m0 + wm * 32 + (lane & 31);
  const int ybytes = M * p.Cout * (kOutBf16 ? 2 : 4);
  const auto ysrc = make_rsrc(p.y, ybytes);
  const auto rsrc = make_rsrc(p.res ? p.res : p.y, ybytes);
  const bool vec = (p.Cout & 3) == 0;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int c = n0 + wn * 32 + 8 * q + 4 * (lane >> 5);
    const f32x4 b = *reinterpret_cast<const f32x4*>(p.bias + c);      // the bias is padded to the tile
    f32x4 v;
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = det_act(acc[4 * q + j], b[j], p.leaky);
    if constexpr (kOutBf16) {      // no residual (the launcher refuses one): 8 bytes a run, or 2 bytes a value where Cout % 4 != 0
      const unsigned lo = pack_bf16x2(v[0], v[1]), hi = pack_bf16x2(v[2], v[3]);
      if (vec) {
        const unsigned off = (pix < M && c < p.Cout) ? ((unsigned)pix * (unsigned)p.Cout + (unsigned)c) * 2u : kOOB;
        __builtin_amdgcn_raw_buffer_store_b64(u32x2{lo, hi}, ysrc, off, 0, 0);
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const unsigned off = (pix < M && c + j < p.Cout) ? ((unsigned)pix * (unsigned)p.Cout + (unsigned)(c + j)) * 2u : kOOB;
          const unsigned word = j < 2 ? lo : hi;
          __builtin_amdgcn_raw_buffer_store_b16((unsigned short)((j & 1) ? word >> 16 : word & 0xffffu), ysrc, off, 0, 0);
        }
      }
    } else if (vec) {
      const unsigned off = (pix < M && c < p.Cout) ? ((unsigned)pix * (unsigned)p.Cout + (unsigned)c) * 4u : kOOB;
      if (p.res) {
        const f32x4 r = load4(rsrc, off);
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = v[j] + r[j];
      }
      buffer_store_b128_sreg(__builtin_bit_cast(u32x4, v), ysrc, off, 0);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const unsigned off = (pix < M && c + j < p.Cout) ? ((unsigned)pix * (unsigned)p.Cout + (unsigned)(c + j)) * 4u : kOOB;
        float o = v[j];
        if (p.res) o = o + __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsrc, off, 0, 0));
        __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, o), ysrc, off, 0, 0);
      }
    }
  }
#endif
}

}  // namespace

int det_conv_launch(const DetConvProblem& p, hipStream_t stream) {
  PR_REQUIRE(p.x && p.w && p.bias && p.y, "det_conv: null tensor");
  PR_REQUIRE(p.ksize == 1 || p.ksize == 3, "det_conv: ksize = %d, must be 1 or 3", p.ksize);
  PR_REQUIRE(p.stride == 1 || p.stride == 2, "det_conv: stride = %d, must be 1 or 2", p.stride);
  PR_REQUIRE(p.B >= 1 && p.H >= 1 && p.W >= 1 && p.Cin >= 4 && p.Cin % 4 == 0 && p.Cout >= 1,
             "det_conv: B %d, H %d, W %d, Cin %d (a multiple of 4), Cout %d", p.B, p.H, p.W, p.Cin, p.Cout);
  const int pad = p.ksize / 2;
  PR_REQUIRE(p.Ho == (p.H + 2 * pad - p.ksize) / p.stride + 1 && p.Wo == (p.W + 2 * pad - p.ksize) / p.stride + 1,
             "det_conv: output %d x %d does not belong to input %d x %d, kernel %d, stride %d", p.Wo, p.Ho, p.W, p.H, p.ksize, p.stride);
  PR_REQUIRE(p.cout_pad % kBN == 0 && p.cout_pad >= p.Cout && p.cout_pad - p.Cout < kBN, "det_conv: cout_pad = %d for Cout = %d", p.cout_pad,
             p.Cout);
  PR_REQUIRE(p.kpad % kBK == 0 && p.kpad >= p.ksize * p.ksize * p.Cin && p.kpad - p.ksize * p.ksize * p.Cin < kBK,
             "det_conv: kpad = %d for K = %d", p.kpad, p.ksize * p.ksize * p.Cin);
  const long lim = 0x7fffffffl;
  PR_REQUIRE((long)p.B * p.H * p.W * p.Cin * 4 <= lim && p.M() * p.Cout * 4 <= lim && (long)p.cout_pad * p.kpad * 4 <= lim,
             "det_conv: a tensor of 2 GiB or more (B %d, %d x %d x %d -> %d x %d x %d)", p.B, p.H, p.W, p.Cin, p.Ho, p.Wo, p.Cout);
  const dim3 grid((unsigned)ceil_div(p.M(), (long)kBM), (unsigned)(p.cout_pad / kBN));
  if (p.out_bf16) {
    PR_REQUIRE(!p.res, "det_conv: a residual with bf16 output is not covered");
    hipLaunchKernelGGL(det_conv_kernel<true>, grid, dim3(kThreads), 0, stream, p);
  } else {
    hipLaunchKernelGGL(det_conv_kernel<false>, grid, dim3(kThreads), 0, stream, p);
  }
  return check_launch("det_conv_kernel");
}

}  // namespace pr
