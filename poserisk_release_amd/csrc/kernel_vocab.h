// The device-side vocabulary the kernels share: vector types, the buffer-descriptor word, the LDS-DMA swizzle, the bf16 pack
// helpers, the XCD block remap and the bf16 MFMA steps.  Included by the kernel files themselves, never by common.h:
// compose.hip and jpeg.hip also compile for the host against tests/native/host_shim.h, which stands in for common.h alone.
#pragma once
#include <hip/hip_runtime.h>

namespace pr {

using f32x16 = __attribute__((ext_vector_type(16))) float;
using f32x4 = __attribute__((ext_vector_type(4))) float;
using f32x2 = __attribute__((ext_vector_type(2))) float;
using bf16x8 = __attribute__((ext_vector_type(8))) __bf16;
using bf16x2 = __attribute__((ext_vector_type(2))) __bf16;
using u32x4 = __attribute__((ext_vector_type(4))) unsigned;
using u32x2 = __attribute__((ext_vector_type(2))) unsigned;
using u16x8 = __attribute__((ext_vector_type(8))) unsigned short;
using i16x2 = __attribute__((ext_vector_type(2))) short;
using i16x8 = __attribute__((ext_vector_type(8))) short;
typedef __attribute__((address_space(3))) void lds_void;

// voffset sentinel of a buffer load / store that must not happen: beyond any buffer the launchers accept (every one checks
// its tensors are < 2 GiB), so the hardware's range check returns zeros (writes zeros to LDS for LDS-DMA) or drops the store.
[[maybe_unused]] constexpr unsigned kOOB = 0x80000000u;

// Word 3 of a raw buffer descriptor on gfx950: DATA_FORMAT (bits 18:15) = 4, one 32-bit element; every other field zero -- no
// swizzle, no index stride, a raw range check of the byte offset against num_records.
constexpr int kBufferRsrcFlags = 0x00020000;
template <typename T>
__device__ __forceinline__ auto make_rsrc(T* ptr, int bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(ptr, 0, bytes, kBufferRsrcFlags);
}
template <typename T>
__device__ __forceinline__ auto make_rsrc(const T* ptr, int bytes) { return make_rsrc(const_cast<T*>(ptr), bytes); }

// LDS-DMA source swizzle.  One buffer_load ... lds instruction writes 64 lanes x 16 bytes = 8 unpadded rows of 128 bytes:
// lane l fills PHYSICAL 16-byte slot l & 7 of row 8 g + (l >> 3), g the 8-row group.  Rule: physical slot p of row r holds
// LOGICAL chunk p ^ ((r >> 1) & 7), which makes the fragment reads conflict free; (r >> 1) & 7 = (4 g + (l >> 4)) & 7, and only
// g's parity matters.  This is the logical chunk the lane must FETCH; every ds_read of such a stage applies the same XOR to
// the chunk it wants: (chunk ^ ((row >> 1) & 7)) << 4.  `group` is the wave where waves take the groups of their own parity.
// A macro, not a function: as an inlined function the compiler simplifies it before it sees the caller's lane arithmetic and
// then selects other instructions in ten kernels (conv_fused, conv_wino64, bottleneck64_bf16: profiles/kernel_vocab_isa.txt).
#define PR_DMA_SWIZZLE_SLOT(lane, group) (((lane) & 7) ^ ((4 * ((group) & 1) + ((lane) >> 4)) & 7))

// Two floats -> two bf16 in one word, lo in the low half (one v_cvt_pk_bf16_f32: round to nearest even, NaN stays NaN).
__device__ __forceinline__ unsigned pack_bf16x2(float lo, float hi) {
  return __builtin_bit_cast(unsigned, __builtin_convertvector(f32x2{lo, hi}, bf16x2));
}
// ... with ReLU, applied to the ROUNDED pair as one v_pk_max_i16: a bf16 is negative exactly when its bits are a negative
// int16, and rounding keeps the sign, so round(relu(v)) == relu(round(v)) for every finite v and both infinities, -0
// included.  With the sums in front as one v_pk_add_f32 each: 6 VALU operations per pair instead of 9.
__device__ __forceinline__ unsigned relu_pack_bf16x2(f32x2 v) {
  const i16x2 r = __builtin_bit_cast(i16x2, __builtin_convertvector(v, bf16x2));
  return __builtin_bit_cast(unsigned, __builtin_elementwise_max(r, i16x2{0, 0}));
}

// Bijective block-index remap for the 8 XCDs: the hardware hands consecutive workgroup ids to the XCDs round-robin;
// this gives XCD x the x-th contiguous run of logical blocks, so neighbouring blocks (which share input rows or
// operand tiles) share an L2.  T is never deduced: the arithmetic runs in `long` unless the caller asks for <int> (the tile
// kernels, whose index arithmetic is 32-bit throughout; the 64-bit form costs them five scalar instructions).
template <typename T>
struct xcd_index { using type = T; };
template <typename T = long>
__device__ __forceinline__ T xcd_contiguous_block(typename xcd_index<T>::type bid, typename xcd_index<T>::type nb) {
  const T xcd = bid & 7, q8 = nb >> 3, rr = nb & 7;
  return (xcd < rr ? xcd * (q8 + 1) : rr * (q8 + 1) + (xcd - rr) * q8) + (bid >> 3);
}

// buffer_store_dwordx4 with a SCALAR-REGISTER soffset.  MEASURED on MI355X (round 3, scripts/micro/t_store_hazard.hip and the
// expand_res_bf16 stress test): when the instruction right behind such a store is a VALU write of the store's first data
// register, the NEW value can reach memory (the stored dword came out as the next tile's half-finished arithmetic, on the
// waves that lose the issue arbitration, a few hundred times per 25 M elements).  The ISA's "VMEM store of more than 64
// bits followed by a write of its data VGPRs" hazard; hipcc pads it only when soffset is NOT a register (LLVM
// GCNHazardRecognizer::createsVALUHazard), so a register soffset -- which the kernels use to keep wave-uniform terms out
// of the range-checked vector offset -- needs its own wait states.  The asm below keeps the data registers live and
// unwritten for four more issue slots; it must stay directly behind the store.
template <typename Rsrc>
__device__ __forceinline__ void buffer_store_b128_sreg(u32x4 v, Rsrc rsrc, unsigned voffset, int soffset) {
#if defined(__HIP_DEVICE_COMPILE__)
  __builtin_amdgcn_raw_buffer_store_b128(v, rsrc, voffset, soffset, 0);
  asm volatile("s_nop 3" ::"v"(v) : "memory");
#endif
}

// One bf16 MFMA step of the kernels on v_mfma_f32_32x32x16_bf16 (weights or rows as A, pixels as B).
__device__ __forceinline__ f32x16 mfma_bf16_step(bf16x8 w, bf16x8 x, f32x16 c) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(w, x, c, 0, 0, 0);
#else
  return c;
#endif
}

// ---- a 32 x 32 output tile on v_mfma_f32_16x16x32_bf16 (round 6) ----------------------------------------------------------
// The bf16 kernels were written for v_mfma_f32_32x32x16_bf16: a wave's unit of output is a 32 x 32 tile whose 16 accumulator
// registers hold, on lane (i = lane & 31, h = lane >> 5), column i of rows (e & 3) + 8 (e >> 2) + 4 h.  The chip can hold a
// higher clock on the 16x16x32 shape at equal cycles per FLOP (MI355X_MICROARCH.md, DVFS give-back 7).  Measured on these
// kernels (profiles/r06_experiments.txt 1): the TILE kernel (conv_dma_bf16) is level to 6 % faster per layer on it and uses it;
// the whole-block kernels were converted the same way, bit for bit, ran 1 - 5 % faster stand-alone (cycles + 4 %, clock + 10 %)
// and 4 - 6 % SLOWER inside the encoder (an MFMA of this shape holds its SIMD's issue port for half its cycles, and in the
// pipeline the clock does not rise), and stay on 32x32x16.  (An earlier estimate of + 5 % end to end, from an experiment build
// that issued each 32x32x16 step as two 16x16x32 MFMAs on alternating accumulator quarters, was WRONG: its wrong results
// changed the data the chip switches on.)  A K loop on this shape issues FOUR 16x16x32 MFMAs per 32 k on the
// tile's four 16 x 16 quadrants -- the same operand bytes from LDS, the same accumulator registers -- and converts ONCE, in
// front of the epilogue, with 8 v_permlane32_swap_b32: afterwards register e of lane l is column i of row
// (e & 3) + 8 (e >> 2) + 4 h for
//     i = 16 (l >> 5) + (l & 15),   h = (l >> 4) & 1        (acc_col / acc_half below)
// i.e. exactly the 32x32x16 registers on relabelled lanes, so every epilogue keeps its arithmetic and only takes (i, h) from
// these two functions.  Measured (scripts/micro/t_mfma16_swap.hip): no element misplaced, and on random bf16 data the sums
// have the 32x32x16 form's BITS (both shapes add the 32 products of a step in the same order).
// Operands of one step: lane (j = l & 15, g = l >> 4) supplies A[row 16 rt + j][k = 8 g .. 8 g + 7] and
// B[k = 8 g .. 8 g + 7][col 16 ct + j] of the step's 32 k (frag_row / frag_kblock below).
struct Acc32 {
  f32x4 t[2][2];   // [rt: rows 16 rt ..][ct: columns 16 ct ..]
};
__device__ __forceinline__ int frag_row(int lane) { return lane & 15; }      // + 16 rt (A) / + 16 ct (B)
__device__ __forceinline__ int frag_kblock(int lane) { return lane >> 4; }   // 8 k each
__device__ __forceinline__ int acc_col(int lane) { return 16 * (lane >> 5) + (lane & 15); }
__device__ __forceinline__ int acc_half(int lane) { return (lane >> 4) & 1; }
__device__ __forceinline__ void acc32_zero(Acc32& c) {
#pragma unroll
  for (int rt = 0; rt < 2; ++rt)
#pragma unroll
    for (int ct = 0; ct < 2; ++ct) c.t[rt][ct] = f32x4{0.f, 0.f, 0.f, 0.f};
}
__device__ __forceinline__ void mfma_bf16_32x32x32(Acc32& c, bf16x8 a0, bf16x8 a1, bf16x8 b0, bf16x8 b1) {
#if defined(__HIP_DEVICE_COMPILE__)
  c.t[0][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0, b0, c.t[0][0], 0, 0, 0);
  c.t[0][1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0, b1, c.t[0][1], 0, 0, 0);
  c.t[1][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1, b0, c.t[1][0], 0, 0, 0);
  c.t[1][1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1, b1, c.t[1][1], 0, 0, 0);
#endif
}
// The tile's accumulators in the 32x32x16 register layout (lane labels acc_col / acc_half).  ONE asm statement: every
// accumulator is an operand, so all the tile's MFMAs have issued in front of it, and the pad in front is the matrix pipe's
// write -> VALU read wait (18 wait states cover a 16-pass MFMA; hipcc pads nothing for asm operands).  The builtin
// __builtin_amdgcn_permlane32_swap is not used: hipcc 7.2 drops its second result and merges calls in exactly this pattern.
__device__ __forceinline__ f32x16 acc32_regs(const Acc32& c) {
  f32x16 o = {};
#if defined(__HIP_DEVICE_COMPILE__)
  float x[8], y[8];
#pragma unroll
  for (int rt = 0; rt < 2; ++rt)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      x[4 * rt + r] = c.t[rt][0][r];
      y[4 * rt + r] = c.t[rt][1][r];
    }
  asm volatile("s_nop 15\n\ts_nop 3\n\t"
               "v_permlane32_swap_b32 %0, %8\n\tv_permlane32_swap_b32 %1, %9\n\tv_permlane32_swap_b32 %2, %10\n\t"
               "v_permlane32_swap_b32 %3, %11\n\tv_permlane32_swap_b32 %4, %12\n\tv_permlane32_swap_b32 %5, %13\n\t"
               "v_permlane32_swap_b32 %6, %14\n\tv_permlane32_swap_b32 %7, %15"
               : "+v"(x[0]), "+v"(x[1]), "+v"(x[2]), "+v"(x[3]), "+v"(x[4]), "+v"(x[5]), "+v"(x[6]), "+v"(x[7]),
                 "+v"(y[0]), "+v"(y[1]), "+v"(y[2]), "+v"(y[3]), "+v"(y[4]), "+v"(y[5]), "+v"(y[6]), "+v"(y[7]));
#pragma unroll
  for (int rt = 0; rt < 2; ++rt)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      o[8 * rt + r] = x[4 * rt + r];
      o[8 * rt + 4 + r] = y[4 * rt + r];
    }
#endif
  return o;
}

}  // namespace pr
