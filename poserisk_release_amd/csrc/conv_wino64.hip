// A 64 -> 64 channel 3x3 / stride-1 / pad-1 fp32 convolution as Winograd F(4x4,3x3) in ONE launch (SPIN Bottleneck conv2 of
// layer1, 56x56 maps; call site lib/core/base.py:220), optionally with the block's 1x1 expansion behind it:
//
//   t2 = relu(A^T [ sum_ci U_k[co][ci] (B^T d B)_k[ci] ] A + b2)      36 products per 4x4 output tile instead of 144
//   y  = relu(t2 * W3^T + b3 + x)                                      (FUSE3: conv3 + bn3 + add + relu, as conv_fused.hip)
//
// The three-launch form (conv_winograd.hip) writes V and M to HBM: 36 planes x 12 544 tiles x 64 channels = 115.6 MB each
// way per layer at B = 64, more than the MFMAs it saves are worth.  Here neither exists outside the CU.
//
// A workgroup (four waves) owns one UNIT: up to 16 horizontally adjacent tiles of one tile row of one frame (56x56: the whole
// row, 14 tiles) x all 64 output channels x all 36 planes.  The 64 input channels pass in four slices of 16:
//
//   1. every thread transforms one (tile, channel) patch of 6x6 in registers (bt6<PTS> down the columns, then along the
//      rows; halo pixels are zeros from the buffer range check) and lays its 36 values into the slice's V image in LDS;
//   2. wave w multiplies, plane by plane, U_k[16 w .. 16 w + 15][slice] (A operand, straight from L2: host_plan packs U per
//      slice so that a wave's fragment of a plane is one contiguous KB) with V_k[slice][16 tiles] (B operand) on
//      v_mfma_f32_16x16x4_f32, three planes in flight (the instruction's dependent latency is 40 cycles, its issue 32);
//   3. a lane's four accumulator values are four consecutive channels of ONE tile for every plane, so the output transform
//      is lane-local: a row of six planes -> four values (at6<PTS>), then column i of A^T into the 16 outputs.  It is
//      accumulated plane row by plane row, slice by slice: 64 registers of y instead of 144 of M.
//
// Every reduction order is fixed by the layer's shape (slice, plane row, k-step, the MFMA's own k order) and a unit never
// spans frames: a frame's bits do not depend on its batch or its place in it.
//
// FUSE3: the unit's t2 (bias, ReLU, rounded to fp32 as the store to HBM would) goes to LDS in conv_fused.hip's operand
// layout, eight tiles = 128 pixels at a time over the V image, and is multiplied by W3 on the 32x32x2 MFMA loop of that
// file: W3 streams through the same two-stage ring, each stage feeding both 64-pixel halves; y leaves from the
// accumulators with the residual.
#include "conv_igemm.h"
#include "kernel_vocab.h"
#include "wino_transforms.h"

namespace pr {
namespace {

constexpr int kTiles = 16;                       // tiles per unit: the B columns of a 16x16x4 MFMA
constexpr int kSlice = 16;                       // input channels per pass
constexpr int kPlane = kTiles * kSlice;          // floats of one plane of the V image
constexpr int kVBytes = 36 * kPlane * 4;         // 36 KB
[[maybe_unused]] constexpr int kRing = kVBytes;  // FUSE3: W3 ring, 2 stages of 64 rows x 128 B
constexpr int kLdsPlain = kVBytes, kLdsFused = kVBytes + 2 * 8192;
// Ring of U fragments (three-plane groups; 12 % kADepth == 0).  Measured: 2 and 3 level, 4 spills; two tile rows per unit
// (eight waves sharing every U fragment) slower (profiles/wino_layer1.txt section 2).
constexpr int kADepth = 2;
static_assert(12 % kADepth == 0, "the ring position of a group must not depend on the slice");
static_assert(2 * 16384 <= kVBytes, "the t2 image of eight tiles lies over the V image");

struct WArgs {
  const float* x;      // t1 [B,H,W,64]
  const float* u;      // [36][4 slices][64 co][16 ci]  (conv_wino64_pack_u)
  const float* bias2;  // [64]
  const float* w3;     // [N3][64] packed, BN folded            (FUSE3)
  const float* bias3;  // [N3]
  const float* res;    // [M][N3] or nullptr
  float* y;            // [M][64], or [M][N3] with FUSE3
  unsigned x_bytes, y_bytes, w3_bytes;
  int H, W, th, tcw, N3, relu, relu3;
};

// Position of (tile, ci = 4 g + e) in a plane of the V image: the lane (tile, g) of an MFMA reads its four k-steps as one
// 16-byte word, the 64 lanes of that read and the 64 lanes of a transform wave's write (4 tiles x 16 channels) each
// cover all 64 banks once.
__device__ __forceinline__ int v_pos(int tile, int g) { return g * 64 + ((4 * tile + 16 * g) & 63); }

template <int PTS, bool FUSE3>
__global__ __launch_bounds__(256, 2) void conv3x3_wino64_f32(const WArgs a) {
#if defined(__HIP_DEVICE_COMPILE__)
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int unit = (int)xcd_contiguous_block(blockIdx.x, gridDim.x);      // neighbouring tile rows share halo rows: one L2
  const int cc = unit % a.tcw, rowid = unit / a.tcw;
  const int ty = rowid % a.th, img = rowid / a.th;
  const int tx0 = cc * kTiles;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);      // output channels 16 wave .. 16 wave + 15
  const auto xsrc = make_rsrc(a.x, (int)a.x_bytes);

  // ---- input transform: thread = (tile pj, channel pc of the slice) -------------------------------------------------
  const int pj = tid >> 4, pc = tid & 15;
  const int h0 = 4 * ty - 1, w0 = 4 * (tx0 + pj) - 1;
  // byte offset of the patch's corner (slice 0); pixels outside the image get the out-of-range sentinel and read as zero
  const int pbase = (((img * a.H + h0) * a.W + w0) * 64 + pc) * 4;
  bool hok[6], wok[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    hok[i] = (unsigned)(h0 + i) < (unsigned)a.H;
    wok[i] = (unsigned)(w0 + i) < (unsigned)a.W;
  }
  float* const vw = reinterpret_cast<float*>(smem) + v_pos(pj, pc >> 2) + (pc & 3);

  // ---- MFMA: lane = (tile j | row i of the A fragment, k group g) ---------------------------------------------------
  const int j = lane & 15, g = lane >> 4;
  // U through a buffer descriptor: one lane offset, the (plane, slice) term in the scalar offset
  const auto usrc = make_rsrc(a.u, 36 * 64 * 64 * 4);
  const int ua = ((16 * wave + j) * kSlice + 4 * g) * 4;      // + (plane * 4 + slice) * 64 * 16 * 4
  const float* const vr = reinterpret_cast<const float*>(smem) + v_pos(j, g);
  f32x4 y[4][4];      // [output row][output column] x four consecutive channels 16 wave + 4 g ..
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c) y[r][c] = f32x4{0.f, 0.f, 0.f, 0.f};

  // U runs ahead of the MFMAs: three-plane group G + kADepth - 1 is requested while group G multiplies (12 groups per slice).
  // The patch is NOT requested a slice ahead: its 36 registers across the MFMA phase spill (profiles/wino_layer1.txt).
  auto load_patch = [&](float (&d)[6][6], int sl) {
    int pb = pbase + sl * kSlice * 4;
    asm volatile("" : "+v"(pb));      // the 36 offsets are recomputed per slice instead of living in 36 registers
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
      for (int jj = 0; jj < 6; ++jj)
        d[i][jj] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(
                                                 xsrc, (hok[i] & wok[jj]) ? pb + (i * a.W + jj) * 256 : (int)kOOB, 0, 0));
  };
  f32x4 af[kADepth][3];
  auto load_a = [&](int sl, int grp, int buf) {      // planes 3 grp .. 3 grp + 2 of slice sl
#pragma unroll
    for (int t = 0; t < 3; ++t)
      af[buf][t] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(usrc, ua, ((3 * grp + t) * 4 + sl) * (64 * kSlice * 4), 0));
  };
#pragma unroll
  for (int gq = 0; gq + 1 < kADepth; ++gq) load_a(0, gq, gq);
  for (int sl = 0; sl < 64 / kSlice; ++sl) {
    float d[6][6];
    load_patch(d, sl);
    __builtin_amdgcn_sched_barrier(0);      // the last plane row's output transform stays out of the input transform
#pragma unroll
    for (int jj = 0; jj < 6; ++jj) bt6<PTS>(d[0][jj], d[1][jj], d[2][jj], d[3][jj], d[4][jj], d[5][jj]);   // B^T d
#pragma unroll
    for (int i = 0; i < 6; ++i) bt6<PTS>(d[i][0], d[i][1], d[i][2], d[i][3], d[i][4], d[i][5]);           // (B^T d) B
    __syncthreads();      // every wave has finished reading the previous slice's V
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
      for (int jj = 0; jj < 6; ++jj) vw[(6 * i + jj) * kPlane] = d[i][jj];
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      __builtin_amdgcn_sched_barrier(0);      // keeps the unrolled plane rows from being interleaved: register pressure
      f32x4 m[6];
#pragma unroll
      for (int hh = 0; hh < 2; ++hh) {
        const int grp = 2 * i + hh;
        if (grp + kADepth - 1 < 12) load_a(sl, grp + kADepth - 1, (grp + kADepth - 1) % kADepth);
        else if (sl + 1 < 64 / kSlice) load_a(sl + 1, grp + kADepth - 1 - 12, (grp + kADepth - 1) % kADepth);
        f32x4 bf[3];
#pragma unroll
        for (int t = 0; t < 3; ++t) {
          bf[t] = *reinterpret_cast<const f32x4*>(vr + (3 * grp + t) * kPlane);
          m[3 * hh + t] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
          for (int t = 0; t < 3; ++t)
            m[3 * hh + t] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[grp % kADepth][t][e], bf[t][e], m[3 * hh + t], 0, 0, 0);
      }
      f32x4 s[4];      // plane row i through A along the columns ...
      at6<PTS>(m[0], m[1], m[2], m[3], m[4], m[5], s[0], s[1], s[2], s[3]);
#pragma unroll
      for (int r = 0; r < 4; ++r) {      // ... and column i of A^T into the four output rows
        constexpr float one = 1.f;
        const float cf = at6_coef<PTS>(r, i);
        if (cf == 0.f) continue;
#pragma unroll
        for (int c = 0; c < 4; ++c) y[r][c] = cf == one ? y[r][c] + s[c] : y[r][c] + cf * s[c];
      }
    }
  }

  const f32x4 b2 = *reinterpret_cast<const f32x4*>(a.bias2 + 16 * wave + 4 * g);
  const auto ysrc = make_rsrc(a.y, (int)a.y_bytes);
  if constexpr (!FUSE3) {
    // ---- t2 = act(y + b2): 16 bytes per lane and pixel, pixels outside the map dropped by the range check -------------
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int ho = 4 * ty + r, wo = 4 * (tx0 + j) + c;
        f32x4 v = y[r][c] + b2;
        if (a.relu) {
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = fmaxf(v[e], 0.f);
        }
        const int off = (((img * a.H + ho) * a.W + wo) * 64 + 16 * wave + 4 * g) * 4;
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), ysrc, ho < a.H && wo < a.W ? off : (int)kOOB, 0, 0);
      }
  } else {
    // ---- conv3 on the unit's t2, eight tiles (two 64-pixel A tiles) at a time: conv_fused.hip's GEMM 2 ---------------
    const int wm = wave >> 1, wn = wave & 1;
    const int q = PR_DMA_SWIZZLE_SLOT(lane, wave);
    const auto w3src = make_rsrc(a.w3, (int)a.w3_bytes);
    const auto rsrc = make_rsrc(a.res ? a.res : a.y, (int)a.y_bytes);
    // a W3 stage is eight 1 KB pieces (8 rows each): pieces wave and wave + 4 are this wave's
    unsigned b3_off[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) b3_off[i] = (unsigned)(((8 * (wave + 4 * i) + (lane >> 3)) * 64 + q * 4) * 4);
    // W3 step s = 2 * chunk + kstep: rows [64 chunk, 64 chunk + 64) of W3, k in [32 kstep, 32 kstep + 32), through registers
    // into the ring (the stage layout of conv_fused.hip: lane-linear, the swizzle on the source address).  Unlike LDS-DMA
    // this needs no vmcnt(0) before a barrier, so the previous chunk's output stores stay in flight across it.
    f32x4 wreg[2];
    auto load3 = [&](int s) {
      const int soff = ((s >> 1) * 64 * 64 + (s & 1) * kConvBK) * 4;
#pragma unroll
      for (int i = 0; i < 2; ++i)
        wreg[i] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(w3src, (int)b3_off[i], soff, 0));
    };
    auto put3 = [&](int s) {
      char* stage = smem + kRing + (s & 1) * 8192;
#pragma unroll
      for (int i = 0; i < 2; ++i) *reinterpret_cast<f32x4*>(stage + (wave + 4 * i) * 1024 + lane * 16) = wreg[i];
    };
    const int frow = lane & 31, fh = lane >> 5, fsw = (frow >> 1) & 7;
    int foff[kConvBK / 8];
#pragma unroll
    for (int kk = 0; kk < kConvBK / 8; ++kk) foff[kk] = frow * 128 + (((2 * kk + fh) ^ fsw) << 4);
    const int nsteps = (a.N3 >> 6) * 2;
    const int col_l = lane & 31;
    for (int hf = 0; hf < 2; ++hf) {
      __syncthreads();      // the V image (hf = 0) / the first eight tiles' t2 and the ring (hf = 1) are consumed
      load3(0);
      if ((j >> 3) == hf) {
        // A-tile row of pixel (r, c) of tile j: 16 (j & 3) + 4 r + c of A tile (j & 7) >> 2; this lane's four channels are
        // 16-byte chunk 4 (wave & 1) + g of K-step wave >> 1 (the stage layout: 128-byte rows, swizzled chunks)
        char* t2 = smem + ((j & 7) >> 2) * 16384 + (wave >> 1) * 8192;
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            const int row = 16 * (j & 3) + 4 * r + c;
            f32x4 v = y[r][c] + b2;
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = fmaxf(v[e], 0.f);
            *reinterpret_cast<f32x4*>(t2 + row * 128 + (((4 * (wave & 1) + g) ^ ((row >> 1) & 7)) << 4)) = v;
          }
      }
      // fragment register e of A tile `sub` is pixel (fh + 2 ((e >> 2) & 1), e & 3) of tile 8 hf + 4 sub + 2 wm + (e >> 3)
      int frag_off[2];      // byte offset of register 0's pixel, column wn * 32 + col_l
      bool cok[2][2][4];    // [sub][e >> 3][e & 3]: the pixel's column lies in the map
      const int ho0 = 4 * ty + fh;
#pragma unroll
      for (int sub = 0; sub < 2; ++sub) {
        const int wo0 = 4 * (tx0 + 8 * hf + 4 * sub + 2 * wm);
        frag_off[sub] = (((img * a.H + ho0) * a.W + wo0) * a.N3 + wn * 32 + col_l) * 4;
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
          for (int c = 0; c < 4; ++c) cok[sub][t][c] = wo0 + 4 * t + c < a.W;
      }
      const bool rok[2] = {ho0 < a.H, ho0 + 2 < a.H};
      put3(0);
      load3(1);
      f32x16 acc[2];
      float rfrag[2][16];
      for (int s = 0; s < nsteps; ++s) {
        __syncthreads();      // W3 stage s is in the ring; (s = 0) the t2 image is complete; stage s-1 is consumed
        if (s + 1 < nsteps) put3(s + 1);
        if (s + 2 < nsteps) load3(s + 2);
        const int n0 = (s >> 1) * 64;
        if ((s & 1) == 0) {
#pragma unroll
          for (int sub = 0; sub < 2; ++sub) {
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[sub][e] = 0.f;
            if (a.res) {
#pragma unroll
              for (int e = 0; e < 16; ++e)      // pixels outside the map get the out-of-range vector offset: they read as zero
                rfrag[sub][e] = __builtin_bit_cast(
                    float, __builtin_amdgcn_raw_buffer_load_b32(
                               rsrc, rok[(e >> 2) & 1] && cok[sub][e >> 3][e & 3] ? frag_off[sub] : (int)kOOB,
                               (n0 + ((2 * ((e >> 2) & 1) * a.W + 4 * (e >> 3) + (e & 3)) * a.N3)) * 4, 0));
            }
          }
        }
        {
          const char* Bb = smem + kRing + (s & 1) * 8192 + wn * 32 * 128;
          const char* Ab = smem + (s & 1) * 8192 + wm * 32 * 128;
          f32x4 af0[kConvBK / 8], af1[kConvBK / 8], bf[kConvBK / 8];
#pragma unroll
          for (int kk = 0; kk < kConvBK / 8; ++kk) {
            af0[kk] = *reinterpret_cast<const f32x4*>(Ab + foff[kk]);
            af1[kk] = *reinterpret_cast<const f32x4*>(Ab + 16384 + foff[kk]);
            bf[kk] = *reinterpret_cast<const f32x4*>(Bb + foff[kk]);
          }
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int kk = 0; kk < kConvBK / 8; ++kk)
#pragma unroll
            for (int jx = 0; jx < 4; ++jx) {
              acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(af0[kk][jx], bf[kk][jx], acc[0], 0, 0, 0);
              acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(af1[kk][jx], bf[kk][jx], acc[1], 0, 0, 0);
            }
        }
        if (s & 1) {
          const float b3 = a.bias3[n0 + wn * 32 + col_l];
#pragma unroll
          for (int sub = 0; sub < 2; ++sub)
#pragma unroll
            for (int e = 0; e < 16; ++e) {      // stores to pixels outside the map get the out-of-range vector offset
              float v = acc[sub][e] + b3;
              if (a.res) v += rfrag[sub][e];
              if (a.relu3) v = fmaxf(v, 0.f);
              __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), ysrc,
                                                    rok[(e >> 2) & 1] && cok[sub][e >> 3][e & 3] ? frag_off[sub] : (int)kOOB,
                                                    (n0 + ((2 * ((e >> 2) & 1) * a.W + 4 * (e >> 3) + (e & 3)) * a.N3)) * 4, 0);
            }
        }
      }
    }
  }
#endif
}

template <int PTS>
int launch_pts(const WArgs& a, bool fuse3, int units, hipStream_t stream) {
  if (fuse3) hipLaunchKernelGGL((conv3x3_wino64_f32<PTS, true>), dim3(units), dim3(256), kLdsFused, stream, a);      // 52 KB of LDS
  else hipLaunchKernelGGL((conv3x3_wino64_f32<PTS, false>), dim3(units), dim3(256), kLdsPlain, stream, a);           // 36 KB
  return check_launch("conv3x3_wino64_f32");
}

}  // namespace

int conv_wino64_launch(const ConvProblem& p, const float* u, int form, hipStream_t stream) {
  PR_REQUIRE(form == 4 || form == 5, "conv_wino64: form %d (4 = F(4x4,3x3) on 0, +-1, +-2; 5 = on 0, +-11/16, +-3/2)", form);
  PR_REQUIRE(p.precision == 0 && p.KH == 3 && p.KW == 3 && p.stride == 1 && p.pad == 1 && p.Ho == p.H && p.Wo == p.W && !p.res &&
                 !p.x2 && p.groups == 1 && p.splitk == 1,
             "conv_wino64: 3x3 / stride 1 / pad 1 fp32 convolutions without residual only");
  PR_REQUIRE(p.Cin == 64 && p.Cout == 64, "conv_wino64: Cin = Cout = 64 only (got %d -> %d)", p.Cin, p.Cout);
  PR_REQUIRE(p.x && u && p.bias && p.B >= 0 && p.H > 0 && p.W > 0, "conv_wino64: needs an input, U and a bias");
  const bool fuse3 = p.w3 != nullptr;
  if (fuse3) PR_REQUIRE(p.bias3 && p.y3 && p.N3 > 0 && p.N3 % 64 == 0, "conv_wino64: conv3 needs a bias and an output with N3 %% 64 == 0 (%d)", p.N3);
  else PR_REQUIRE(p.y, "conv_wino64: null output");
  const int nout = fuse3 ? p.N3 : 64;
  const size_t xb = (size_t)p.B * p.H * p.W * 64 * 4, yb = (size_t)p.M() * nout * 4;
  PR_REQUIRE(xb < (1ull << 31) && yb < (1ull << 31), "conv_wino64: tensor too large for one launch");
  WArgs a;
  a.x = p.x; a.u = u; a.bias2 = p.bias; a.w3 = p.w3; a.bias3 = p.bias3; a.res = fuse3 ? p.res3 : nullptr; a.y = fuse3 ? p.y3 : p.y;
  a.x_bytes = (unsigned)xb; a.y_bytes = (unsigned)yb; a.w3_bytes = fuse3 ? (unsigned)((size_t)p.N3 * 64 * 4) : 0u;
  a.H = p.H; a.W = p.W; a.th = (p.H + 3) / 4; a.tcw = ((p.W + 3) / 4 + kTiles - 1) / kTiles; a.N3 = p.N3; a.relu = p.relu; a.relu3 = p.relu3;
  const long units = (long)p.B * a.th * a.tcw;
  PR_REQUIRE(units < (1L << 31), "conv_wino64: %ld units are too many for one launch", units);
  if (units == 0) return PR_OK;
  return form == 5 ? launch_pts<1>(a, fuse3, (int)units, stream) : launch_pts<0>(a, fuse3, (int)units, stream);
}

}  // namespace pr
