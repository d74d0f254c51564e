// A whole ResNet-50 Bottleneck of layer1 (64 planes at 56x56) in ONE persistent bf16 kernel:
//   y = relu( bn3(conv3( relu(bn2(conv2_3x3( relu(bn1(conv1(x))) ))) )) + x )        x, y: [M = B*H*W][256] bf16 NHWC
// (SPIN models/hmr.py Bottleneck.forward, restated in oracle/hmr_ref.py; call site lib/core/base.py:220).
//
// Why one kernel: as three launches the block moves 1.44 GB at B=256 (x read twice, the two 64-channel maps written
// and read back) and every 64-row workgroup is a chain of ~17 serial waits; fused it moves x in and y out (822 MB) and
// the next pixels' loads are in flight while the current ones compute.
//
// Structure (one workgroup of 4 waves per CU, one wave per SIMD, up to 512 VGPRs each):
//   * A workgroup walks a contiguous run of 64-pixel blocks of the flattened [B*H*W] pixel index.  conv1 of block
//     t+2 is computed while block t is finished, so the 3x3 conv2 of block t finds t1 = relu(conv1(x)) of blocks
//     t-1, t, t+1 (its +-(W+1) pixel neighbourhood, W <= 63) in a three-block LDS ring: every pixel's conv1 is computed once
//     per workgroup (two extra blocks per run), no halo tiles.  Zero padding = per-lane tap masks (a masked lane reads a zero row).
//   * The MFMAs run "transposed": the weights are the A operand (rows = output channels), the pixels the B operand, so an
//     accumulator lane IS a pixel and its 16 registers are 16 consecutive channels (the packed weight rows are permuted
//     for that on the host).  t1 / t2 go to LDS and y to HBM straight from the registers as 16-byte pieces: no LDS
//     transpose, no epilogue barrier.
//   * W2 (72 KB) stays in LDS for the whole kernel; W1 and W3 (32 KB each) stay in REGISTERS as MFMA A fragments
//     (each wave holds the rows of its own output tiles: 64 + 64 VGPRs); biases in LDS.
//   * x streams through a six-slice LDS ring by LDS-DMA (a slice = 64 pixels x 64 channels = 8 KB), issued 1.5 blocks
//     ahead; the block's own rows are picked out of the ring into registers as the residual when conv1 consumes them
//     (x is read from HBM exactly once).
//   * Same k order and the same 16-wide MFMA groups as conv_dma_bf16 / conv3x3_conv1x1_bf16, t1 and t2 rounded to bf16
//     exactly where the separate launches store them.
#include <algorithm>
#include <cstdlib>

#include "conv_igemm.h"
#include "kernel_vocab.h"
#include "timing_hooks.h"

namespace pr {
namespace {

constexpr int kRing = 192;                         // t1 ring: three 64-pixel blocks
constexpr int kXSlots = 6;                         // x ring: six 8 KB slices
constexpr int kRowT = 144;                         // t1 / t2 row: 64 channels + 16 bytes of padding (conflict-free b128 reads)
constexpr int kOffW2 = 0;                          // 9 taps x [64 rows][64 k] bf16, 16-byte chunks XOR-swizzled
constexpr int kOffT1 = 9 * 8192;                   // [192 pixels] rows of kRowT
constexpr int kOffT2 = kOffT1 + kRing * kRowT;     // [64 pixels] rows of kRowT
constexpr int kOffX = kOffT2 + 64 * kRowT;         // kXSlots x [64 pixels][64 channels] bf16, XOR-swizzled
constexpr int kOffB1 = kOffX + kXSlots * 8192;     // 64 floats
constexpr int kOffB2 = kOffB1 + 256;               // 64 floats
constexpr int kOffB3 = kOffB2 + 256;               // 256 floats
constexpr int kOffZero = kOffB3 + 1024;            // 512 zero bytes: what a masked conv2 tap reads (from the bank of the lane's own row)
constexpr int kLdsBytes = kOffZero + 512;
static_assert(kLdsBytes <= 160 * 1024 && kOffX % 1024 == 0, "LDS budget / DMA alignment");

struct BnArgs {
  const unsigned short* x;
  unsigned short* y;
  const unsigned short* w1;   // [64][256]  rows permuted (bottleneck_pack_rows_bf16)
  const unsigned short* w2;   // [64][576]  rows permuted, k = tap * 64 + c1
  const unsigned short* w3;   // [256][64]  rows permuted
  const float* b1;            // true channel order
  const float* b2;
  const float* b3;
  unsigned x_bytes, y_bytes;
  int H, W, HW, M, nblocks;
  unsigned long long* stamps;   // timing builds only (-DPR_TIMING_HOOKS): s_memtime at the phase boundaries of iterations 8 .. 23
};
constexpr int kStampJ0 = 8, kStampNJ = 16, kStampK = 6;

#define PR_BARRIER()                                         \
  do {                                                       \
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");       \
    __builtin_amdgcn_s_barrier();                            \
    asm volatile("" ::: "memory");                           \
  } while (0)

// DBG (timing builds only, -DPR_TIMING_HOOKS; results are wrong when set): 1 no y stores, 2 y stores ADDRESSED as 8 rows x 128 B
// per instruction (what an LDS transpose in front of them could return at most), 4 no MFMAs, 8 no x loads.
// FIRST: the stage's first block -- x has 64 channels (one slice per block), conv3 and the downsample branch are one GEMM
// over K = [t2's 64 channels | x's 64 channels] (w3 = [256][128], b3 = both folded biases summed), and there is no
// residual: group B picks x's rows out of the ring as MFMA B fragments instead of as packed residual values.
template <int DBG, bool FIRST>
__global__ __launch_bounds__(512) void bottleneck64_bf16(const BnArgs a) {
#if defined(__HIP_DEVICE_COMPILE__)
  extern __shared__ __attribute__((aligned(16))) char smem[];
  auto MFMA = [](const bf16x8& wa, const bf16x8& xb, const f32x16& c) -> f32x16 {
    if (DBG & 4) {                                   // keep the operands live so nothing upstream is removed
      asm volatile("" ::"v"(wa), "v"(xb));
      return c;
    }
    return mfma_bf16_step(wa, xb, c);
  };
  // s_waitcnt vmcnt(n) for a wave-uniform run-time n (the instruction takes an immediate)
  auto wait_vm = [](int n) {
    switch (n) {
      case 12: asm volatile("s_waitcnt vmcnt(12)" ::: "memory"); break;
      case 11: asm volatile("s_waitcnt vmcnt(11)" ::: "memory"); break;
      case 10: asm volatile("s_waitcnt vmcnt(10)" ::: "memory"); break;
      case 9: asm volatile("s_waitcnt vmcnt(9)" ::: "memory"); break;
      case 8: asm volatile("s_waitcnt vmcnt(8)" ::: "memory"); break;
      case 7: asm volatile("s_waitcnt vmcnt(7)" ::: "memory"); break;
      case 6: asm volatile("s_waitcnt vmcnt(6)" ::: "memory"); break;
      case 5: asm volatile("s_waitcnt vmcnt(5)" ::: "memory"); break;
      case 4: asm volatile("s_waitcnt vmcnt(4)" ::: "memory"); break;
      case 3: asm volatile("s_waitcnt vmcnt(3)" ::: "memory"); break;
      case 2: asm volatile("s_waitcnt vmcnt(2)" ::: "memory"); break;
      case 1: asm volatile("s_waitcnt vmcnt(1)" ::: "memory"); break;
      default: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
    }
  };
  constexpr int SPB = FIRST ? 1 : 4;      // x slices (64 channels, 8 KB in LDS) per 64-pixel block
  constexpr int XROW = FIRST ? 128 : 512; // bytes of an x row
  auto STAMP = [&](int j, int k) {
#ifdef PR_TIMING_HOOKS
    if (a.stamps && j >= kStampJ0 && j < kStampJ0 + kStampNJ && (threadIdx.x & 63) == 0)
      a.stamps[(((size_t)blockIdx.x * 8 + (threadIdx.x >> 6)) * kStampNJ + (j - kStampJ0)) * kStampK + k] = __builtin_amdgcn_s_memtime();
#endif
  };
  const int b0 = (int)((unsigned)blockIdx.x * (unsigned)a.nblocks / gridDim.x);   // nblocks * gridDim < 2^32 (host check)
  const int b1 = (int)(((unsigned)blockIdx.x + 1u) * (unsigned)a.nblocks / gridDim.x);
  if (b0 >= b1) return;                              // the whole workgroup leaves before any barrier
  const int nc = b1 - b0 + 2;                        // conv1 blocks b0-1 .. b1 (local 0 .. nc-1)

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int i = lane & 31, h = lane >> 5;
  const int ct = (wave & 3) >> 1, pt = wave & 1;     // output-channel tile (conv1/conv2) or tile group (conv3), pixel tile
  const int prow = 32 * pt + i;                      // the lane's pixel inside a 64-pixel block

  // ---- one-time loads (all eight waves) ------------------------------------------------------------------------------
  {
    // W2 -> LDS: 9 taps x [64 rows][128 B], 16-byte chunks XOR-swizzled on the source side (conv_dma_bf16.hip); the 72
    // 1 KB groups of 8 rows are dealt to the eight waves
    const auto w2src = make_rsrc(a.w2, 64 * 576 * 2);
    for (int idx = wave; idx < 72; idx += 8) {
      const int tap = idx >> 3, grp = idx & 7;
      const int q = PR_DMA_SWIZZLE_SLOT(lane, grp);
      const unsigned voff = (unsigned)(((8 * grp + (lane >> 3)) * 576 + q * 8) * 2);
      __builtin_amdgcn_raw_ptr_buffer_load_lds(w2src, (lds_void*)(smem + kOffW2 + tap * 8192 + grp * 1024), 16, voff,
                                               tap * 128, 0, 0);
    }
    if (tid < 64) {
      *reinterpret_cast<float*>(smem + kOffB1 + tid * 4) = a.b1[tid];
      *reinterpret_cast<float*>(smem + kOffB2 + tid * 4) = a.b2[tid];
    }
    if (tid < 256) *reinterpret_cast<float*>(smem + kOffB3 + tid * 4) = a.b3[tid];
    if (tid < 128) *reinterpret_cast<unsigned*>(smem + kOffZero + tid * 4) = 0u;
  }

  if (wave < 4) {
    // =================================================================================================================
    // group A (waves 0-3, one per SIMD): the x ring's LDS-DMA, conv2 of block t, then conv1 of block t+2 -- the matrix half
    // =================================================================================================================
    const auto xsrc = make_rsrc(a.x, (int)a.x_bytes);
    bf16x8 w1f[4 * SPB];     // W1 rows of this wave's output tile as MFMA A fragments (row i, k = 16 ks + 8 h .. + 7)
#pragma unroll
    for (int ks = 0; ks < 4 * SPB; ++ks)
      w1f[ks] = *reinterpret_cast<const bf16x8*>(a.w1 + (32 * ct + i) * (64 * SPB) + 16 * ks + 8 * h);
    // x ring: local slice L = 4 * (local conv1 block) + s, s = 64-channel slice of x; LDS slot L % 6.  A slice is eight
    // 1 KB DMA groups of 8 pixels: ONE instruction per slice for each of the eight waves (group = wave; an LDS-DMA
    // instruction costs its wave ~200 cycles of issue, so both groups carry half).
    const int dq = PR_DMA_SWIZZLE_SLOT(lane, wave);
    auto issue_slice = [&](int L) {
      const int blk = b0 - 1 + L / SPB, s = L % SPB;
      const int m = blk * 64 + 8 * wave + (lane >> 3);
      const unsigned voff = (m >= 0 && m < a.M) ? (unsigned)(m * XROW + dq * 16) : kOOB;
      if (!(DBG & 8))
        __builtin_amdgcn_raw_ptr_buffer_load_lds(xsrc, (lds_void*)(smem + kOffX + (L % kXSlots) * 8192 + wave * 1024), 16, voff,
                                                 s * 128, 0, 0);
    };
    int gi = 0;                                      // next slice to issue
    const int nslices = SPB * nc;
    for (; gi < kXSlots && gi < nslices; ++gi) issue_slice(gi);

    // fragment read offsets inside a swizzled [64 rows][128 B] block: the lane's row, logical chunk 2 kk + h
    int pfoff[4], wfoff[4];
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      pfoff[kk] = prow * 128 + (((2 * kk + h) ^ ((prow >> 1) & 7)) << 4);
      wfoff[kk] = (32 * ct + i) * 128 + (((2 * kk + h) ^ ((i >> 1) & 7)) << 4);
    }
    const float invW = 1.0f / (float)a.W;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's rows of W2 (and the first x slices; once)
    PR_BARRIER();

    for (int j = 0; j <= nc + 1; ++j) {
      STAMP(j, 0);
      if (j >= 3 && j <= nc) {
        // ---- conv2 of output block t: t1 of blocks t-1, t, t+1 is in the ring ------------------------------------
        const int t = b0 + j - 3;
        const int m = t * 64 + prow;
        const int rem = m % a.HW;
        const int ho = (int)(((float)rem + 0.5f) * invW), wo = rem - ho * a.W;   // exact: rem < 2^23, fraction >= 0.5 / W
        const int rbase = m % kRing;
        // the nine taps' t1 rows first (a masked tap reads zeros)
        int trow[9];
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
          const int dh = tap / 3 - 1, dw = tap % 3 - 1;
          int R = rbase + dh * a.W + dw;
          R += R < 0 ? kRing : 0;
          R -= R >= kRing ? kRing : 0;
          const bool ok = (unsigned)(ho + dh) < (unsigned)a.H && (unsigned)(wo + dw) < (unsigned)a.W;
          // a masked lane reads its zeros from the bank its own ring row would have used: no collision with the other lanes' rows
          trow[tap] = ok ? kOffT1 + R * kRowT + 16 * h : kOffZero + ((R * kRowT + 16 * h) & 255);
        }
        f32x16 acc;
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[e] = 0.f;
        // One dependent MFMA chain (the k order of the separate launches); the next tap's fragments are requested before the
        // current tap's four MFMAs are issued (one group A wave per SIMD: nothing else would hide the LDS latency).
        bf16x8 af[2][4], bf[2][4];
        auto fetch = [&](int tap, bf16x8* fa, bf16x8* fb) {
#pragma unroll
          for (int kk = 0; kk < 4; ++kk) {
            fb[kk] = *reinterpret_cast<const bf16x8*>(smem + trow[tap] + 32 * kk);
            fa[kk] = *reinterpret_cast<const bf16x8*>(smem + kOffW2 + tap * 8192 + wfoff[kk]);
          }
        };
        fetch(0, af[0], bf[0]);
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
          if (tap + 1 < 9) fetch(tap + 1, af[(tap + 1) & 1], bf[(tap + 1) & 1]);
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int kk = 0; kk < 4; ++kk) acc = MFMA(af[tap & 1][kk], bf[tap & 1][kk], acc);
          __builtin_amdgcn_sched_barrier(0);
        }
        // t2 = bf16(relu(acc + b2)) -> LDS [pixel][channel]; the lane's 16 registers are channels 32 ct + 16 h + r
        const float* bp = reinterpret_cast<const float*>(smem + kOffB2) + 32 * ct + 16 * h;
        unsigned pk[8];
#pragma unroll
        for (int e = 0; e < 8; ++e)
          pk[e] = pack_bf16x2(fmaxf(acc[2 * e] + bp[2 * e], 0.f), fmaxf(acc[2 * e + 1] + bp[2 * e + 1], 0.f));
        char* dst = smem + kOffT2 + prow * kRowT + 64 * ct + 32 * h;
        *reinterpret_cast<u32x4*>(dst) = u32x4{pk[0], pk[1], pk[2], pk[3]};
        *reinterpret_cast<u32x4*>(dst + 16) = u32x4{pk[4], pk[5], pk[6], pk[7]};
      }
      STAMP(j, 1);
      if (j < nc) {
        // This wave's part of block j's slices must have landed.  Vector-memory operations retire in issue order, so it is
        // enough to leave the younger ones in flight: one DMA instruction per slice issued beyond them.
        wait_vm(gi - SPB * (j + 1));
      }
      STAMP(j, 2);
      PR_BARRIER();      // b1: t2 written, group B is done with the previous t2; everyone's slices have landed
      STAMP(j, 3);
      if (j < nc) {
        // ---- conv1 of local block j (global block b0 - 1 + j) -> t1 ring --------------------------------------------
        f32x16 acc;
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[e] = 0.f;
        bf16x8 xf[2][4];
        auto fetchx = [&](int s, bf16x8* f) {
          const char* slot = smem + kOffX + ((SPB * j + s) % kXSlots) * 8192;
#pragma unroll
          for (int kk = 0; kk < 4; ++kk) f[kk] = *reinterpret_cast<const bf16x8*>(slot + pfoff[kk]);
        };
        fetchx(0, xf[0]);
#pragma unroll
        for (int s = 0; s < SPB; ++s) {
          if (s + 1 < SPB) fetchx(s + 1, xf[(s + 1) & 1]);
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int kk = 0; kk < 4; ++kk) acc = MFMA(w1f[4 * s + kk], xf[s & 1][kk], acc);
          __builtin_amdgcn_sched_barrier(0);
        }
        const int m2 = (b0 - 1 + j) * 64 + prow;
        int R = m2 % kRing;
        R += R < 0 ? kRing : 0;
        const float* bp = reinterpret_cast<const float*>(smem + kOffB1) + 32 * ct + 16 * h;
        unsigned pk[8];
#pragma unroll
        for (int e = 0; e < 8; ++e)
          pk[e] = pack_bf16x2(fmaxf(acc[2 * e] + bp[2 * e], 0.f), fmaxf(acc[2 * e + 1] + bp[2 * e + 1], 0.f));
        char* dst = smem + kOffT1 + R * kRowT + 64 * ct + 32 * h;
        *reinterpret_cast<u32x4*>(dst) = u32x4{pk[0], pk[1], pk[2], pk[3]};
        *reinterpret_cast<u32x4*>(dst + 16) = u32x4{pk[4], pk[5], pk[6], pk[7]};
      }
      STAMP(j, 4);
      PR_BARRIER();      // b0: t1 visible; the four slices are free (group B has picked its residual rows out of them)
      STAMP(j, 5);
      for (; gi < SPB * (j + 1) + kXSlots && gi < nslices; ++gi) issue_slice(gi);
    }
  } else {
    // =================================================================================================================
    // group B (waves 4-7, one beside each group A wave): conv3 + residual + ReLU of the block group A finished in the
    // previous iteration, stored from the registers -- the VALU / store half, beside group A's MFMAs on the same SIMDs.
    // Wave (ct, pt) owns the output tiles 4 ct .. 4 ct + 3 (channels 128 ct .. 128 ct + 127) of pixel tile pt.
    // =================================================================================================================
    const auto ysrc = make_rsrc(a.y, (int)a.y_bytes);
    const auto xsrc = make_rsrc(a.x, (int)a.x_bytes);
    // this group's half of the x ring's LDS-DMA (see group A): group `wave` (4..7) of every slice
    const int dq = PR_DMA_SWIZZLE_SLOT(lane, wave);
    auto issue_slice = [&](int L) {
      const int blk = b0 - 1 + L / SPB, s = L % SPB;
      const int m = blk * 64 + 8 * wave + (lane >> 3);
      const unsigned voff = (m >= 0 && m < a.M) ? (unsigned)(m * XROW + dq * 16) : kOOB;
      if (!(DBG & 8))
        __builtin_amdgcn_raw_ptr_buffer_load_lds(xsrc, (lds_void*)(smem + kOffX + (L % kXSlots) * 8192 + wave * 1024), 16, voff,
                                                 s * 128, 0, 0);
    };
    int gi = 0;                                      // next slice to issue
    const int nslices = SPB * nc;
    for (; gi < kXSlots && gi < nslices; ++gi) issue_slice(gi);
    constexpr int K3 = FIRST ? 8 : 4;   // k-steps of conv3 (FIRST: t2's four, then x's four)
    bf16x8 w3f[4][K3];       // W3 rows of this wave's four output tiles
#pragma unroll
    for (int n = 0; n < 4; ++n)
#pragma unroll
      for (int kk = 0; kk < K3; ++kk)
        w3f[n][kk] = *reinterpret_cast<const bf16x8*>(a.w3 + (32 * (4 * ct + n) + i) * (16 * K3) + 16 * kk + 8 * h);
    // Residual rows (packed bf16 pairs, the epilogue's layout): picked out of the x ring when conv1 reads the block
    // (iteration j), used in iterations j + 2 (tile 0) and j + 3 (tiles 1-3).  Three generations are alive; generation
    // g lives in buffer g % 3, and the loop below is unrolled by three so that the buffer is a compile-time choice (no
    // copies): iteration j's tiles 1-3 read buffer j % 3 (picked at j - 3) before its pick-up overwrites it.
    unsigned r0[32], r1[32], r2[32];
#pragma unroll
    for (int e = 0; e < 32; ++e) r0[e] = r1[e] = r2[e] = 0u;
    bf16x8 tf[4];
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) tf[kk] = bf16x8{};
    const int sw = (prow >> 1) & 7;

    // conv3 tile 4 ct + n of block u + bias + residual + ReLU -> y, straight from the accumulator registers
    auto tile = [&](int n, int u, const unsigned* res) {
      f32x16 c3;
#pragma unroll
      for (int e = 0; e < 16; ++e) c3[e] = 0.f;
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) c3 = MFMA(w3f[n][kk], tf[kk], c3);
      if (FIRST) {           // the downsample branch: the block's own x rows as the K loop's second half
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
          const bf16x8 xb = __builtin_bit_cast(bf16x8, u32x4{res[4 * kk], res[4 * kk + 1], res[4 * kk + 2], res[4 * kk + 3]});
          c3 = MFMA(w3f[n][K3 - 4 + kk], xb, c3);
        }
      }
      const float* bp = reinterpret_cast<const float*>(smem + kOffB3) + 32 * (4 * ct + n) + 16 * h;
      unsigned pk[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        float v0 = c3[2 * e] + bp[2 * e], v1 = c3[2 * e + 1] + bp[2 * e + 1];
        if (!FIRST) {
          const unsigned rr = res[8 * n + e];
          v0 += __uint_as_float(rr << 16);
          v1 += __uint_as_float(rr & 0xffff0000u);
        }
        pk[e] = pack_bf16x2(fmaxf(v0, 0.f), fmaxf(v1, 0.f));
      }
      // rows >= M lie beyond the descriptor's range and are dropped by the hardware
      const int m = u * 64 + prow;
      const unsigned yoff = m < a.M ? (unsigned)(m * 512 + 32 * h) : kOOB;
      if (DBG & 1) asm volatile("" ::"v"(pk[0]), "v"(pk[1]), "v"(pk[2]), "v"(pk[3]), "v"(pk[4]), "v"(pk[5]), "v"(pk[6]), "v"(pk[7]));
      if (DBG & 2) {         // timing only (wrong placement): the same bytes addressed as 8 rows x 128 B per instruction
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const int sidx = 2 * n + j;
          const int m2 = u * 64 + 32 * pt + 8 * (sidx & 3) + (lane >> 3);
          const unsigned y2 = m2 < a.M ? (unsigned)(m2 * 512 + 16 * (lane & 7)) : kOOB;
          buffer_store_b128_sreg(u32x4{pk[4 * j], pk[4 * j + 1], pk[4 * j + 2], pk[4 * j + 3]}, ysrc, y2, 256 * ct + 128 * (sidx >> 2));
        }
      } else if (!(DBG & 1)) {
        buffer_store_b128_sreg(u32x4{pk[0], pk[1], pk[2], pk[3]}, ysrc, yoff, 64 * (4 * ct + n));
        buffer_store_b128_sreg(u32x4{pk[4], pk[5], pk[6], pk[7]}, ysrc, yoff + 16, 64 * (4 * ct + n));
      }
    };

    // one iteration: `mine` = buffer j % 3 (tiles 1-3 of block b0 + j - 4, then this iteration's pick-up), `next` =
    // buffer (j + 1) % 3 (picked at j - 2: tile 0 of block b0 + j - 3)
    auto iteration = [&](int j, unsigned* mine, const unsigned* next) {
      STAMP(j, 0);
      // the slices conv1 consumed in the previous iteration are free: refill them
      if (j >= 1)
        for (; gi < SPB * j + kXSlots && gi < nslices; ++gi) issue_slice(gi);
      STAMP(j, 1);
      if (j >= 4) {          // beside group A's conv2 (t2 fragments of that block were read in the previous iteration)
        tile(1, b0 + j - 4, mine);
        tile(2, b0 + j - 4, mine);
        tile(3, b0 + j - 4, mine);
      }
      if (j < nc) {
        // This wave's part of block j's slices must have landed before b1 publishes them.  Vector-memory operations
        // retire in issue order, so the YOUNGER ones may stay in flight: the slices issued beyond them (one instruction
        // each) and, behind those, the six stores of the tiles above (always issued: rows >= M are dropped by the range check).
        wait_vm(gi - SPB * (j + 1) + ((j >= 4 && !(DBG & 1)) ? 6 : 0));
      }
      STAMP(j, 2);
      PR_BARRIER();      // b1
      STAMP(j, 3);
      if (j >= 3 && j <= nc) {   // t2 of block t = b0 + j - 3 (this pixel tile, all 64 channels) as MFMA B fragments
#pragma unroll
        for (int kk = 0; kk < 4; ++kk)
          tf[kk] = *reinterpret_cast<const bf16x8*>(smem + kOffT2 + prow * kRowT + 32 * kk + 16 * h);
      }
      if (j < nc) {
        if (FIRST) {
          // the rows of local block j as conv3's second B operand: this pixel tile's row, logical chunk 2 kk + h
          const char* base = smem + kOffX + (j % kXSlots) * 8192 + prow * 128;
#pragma unroll
          for (int kk = 0; kk < 4; ++kk) {
            const u32x4 v = *reinterpret_cast<const u32x4*>(base + (((2 * kk + h) ^ sw) << 4));
#pragma unroll
            for (int e = 0; e < 4; ++e) mine[4 * kk + e] = v[e];
          }
        } else {
          // the rows of local block j (output block b0 - 1 + j) in the conv3 epilogue's layout: tile 4 ct + n -> channels
          // 32 (4 ct + n) + 16 h .. + 15, i.e. slice 2 ct + (n >> 1), logical chunks 4 (n & 1) + 2 h and + 1
#pragma unroll
          for (int n = 0; n < 4; ++n) {
            const int cl = 4 * (n & 1) + 2 * h;
            const char* base = smem + kOffX + ((4 * j + 2 * ct + (n >> 1)) % kXSlots) * 8192 + prow * 128;
            const u32x4 lo = *reinterpret_cast<const u32x4*>(base + ((cl ^ sw) << 4));
            const u32x4 hi = *reinterpret_cast<const u32x4*>(base + (((cl + 1) ^ sw) << 4));
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              mine[8 * n + e] = lo[e];
              mine[8 * n + 4 + e] = hi[e];
            }
          }
        }
      }
      if (j >= 3 && j <= nc) tile(0, b0 + j - 3, next);   // beside group A's conv1
      STAMP(j, 4);
      PR_BARRIER();      // b0
      STAMP(j, 5);
    };

    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's rows of W2
    PR_BARRIER();
    for (int j = 0; j <= nc + 1; j += 3) {
      iteration(j, r0, r1);
      if (j + 1 <= nc + 1) iteration(j + 1, r1, r2);
      if (j + 2 <= nc + 1) iteration(j + 2, r2, r0);
    }
  }
#endif
}
#undef PR_BARRIER

}  // namespace

// (bottleneck_pack_rows_bf16 -- the row permutation sigma of these transposed MFMAs -- lives in host_plan.cc)
int bottleneck_bf16_launch(const BottleneckProblem& p, hipStream_t stream) {
  if (p.planes == 128) return bottleneck128_bf16_launch(p, stream);
  if (p.planes == 256) return bottleneck256_bf16_launch(p, stream);
  PR_REQUIRE(p.x && p.y && p.w1 && p.w2 && p.w3 && p.b1 && p.b2 && p.b3, "bottleneck: null argument");
  PR_REQUIRE(p.planes == 64, "bottleneck: 64 planes only (got %d)", p.planes);
  PR_REQUIRE(p.W >= 1 && p.W <= 63 && p.H >= 1, "bottleneck: map %dx%d unsupported (width 1..63)", p.H, p.W);
  const long M = (long)p.B * p.H * p.W;
  PR_REQUIRE(M * 512 < (1L << 31), "bottleneck: tensor too large for one launch (%ld pixels)", M);   // also keeps nblocks * grid < 2^32
  if (M == 0) return PR_OK;
  BnArgs a;
  a.x = reinterpret_cast<const unsigned short*>(p.x); a.y = reinterpret_cast<unsigned short*>(p.y);
  a.w1 = reinterpret_cast<const unsigned short*>(p.w1); a.w2 = reinterpret_cast<const unsigned short*>(p.w2);
  a.w3 = reinterpret_cast<const unsigned short*>(p.w3);
  a.b1 = p.b1; a.b2 = p.b2; a.b3 = p.b3;
  a.x_bytes = (unsigned)(M * (p.first ? 128 : 512));
  a.y_bytes = (unsigned)(M * 512);
  a.H = p.H; a.W = p.W; a.HW = p.H * p.W; a.M = (int)M; a.nblocks = (int)ceil_div(M, 64L);
  int cus = 256;
  PR_TRY(current_device_cus(&cus));
  const int grid = std::min(cus, a.nblocks);
  void (*kern)(const BnArgs) = p.first ? bottleneck64_bf16<0, true> : bottleneck64_bf16<0, false>;
  a.stamps = nullptr;
#ifdef PR_TIMING_HOOKS
  static int stamp_calls = 0;   // the 30th call: a warm launch in the middle of the timing loop
  StampRecorder stamp_rec("POSERISK_BN_STAMPS", (size_t)256 * 8 * kStampNJ * kStampK, 30, stamp_calls, stream);
  a.stamps = stamp_rec.stamps();
  if (const char* e = getenv("POSERISK_BN_DBG")) {
    switch (atoi(e)) {
      case 1: kern = p.first ? bottleneck64_bf16<1, true> : bottleneck64_bf16<1, false>; break;
      case 2: kern = p.first ? bottleneck64_bf16<2, true> : bottleneck64_bf16<2, false>; break;
      case 4: kern = p.first ? bottleneck64_bf16<4, true> : bottleneck64_bf16<4, false>; break;
      case 5: kern = p.first ? bottleneck64_bf16<5, true> : bottleneck64_bf16<5, false>; break;
      case 13: kern = p.first ? bottleneck64_bf16<13, true> : bottleneck64_bf16<13, false>; break;
    }
    PR_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, kLdsBytes));
  }
#endif
  static std::atomic<uint64_t> attr_done{0}, attr_done_first{0};
  if (p.first) PR_TRY(ensure_dynamic_lds(reinterpret_cast<const void*>(bottleneck64_bf16<0, true>), kLdsBytes, attr_done_first));
  else PR_TRY(ensure_dynamic_lds(reinterpret_cast<const void*>(bottleneck64_bf16<0, false>), kLdsBytes, attr_done));
  hipLaunchKernelGGL(kern, dim3(grid), dim3(512), kLdsBytes, stream, a);
  return check_launch("bottleneck64_bf16");
}

}  // namespace pr
