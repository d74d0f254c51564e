// Device half of the PNG encoder: u8 frames on the device -> complete PNG files in per-frame slots.  The contract is written in
// include/poserisk_hip.h (section j5); the logic is csrc/png_enc_device.h, instantiated here for 64 lanes;
// tests/png_enc_ref.py restates it, tests/test_png_encode_native.py runs the one-lane form under sanitizers and
// tests/test_png_encode_gpu.py compares every byte of this file's output with the reference.
//
//   choose    adaptive only.  One wavefront per row: the five filters' sums of |signed byte|, the row's filter byte.
//   segment   one wavefront (one workgroup) per 16 KiB segment: its filtered bytes straight from the pixels into LDS -- the
//             filtered stream never exists in memory --, run starts by ballot, tokens, histogram, code lengths and codes, every
//             token's bits at its prefix-summed offset, or the stored block; the CRC register and the Adler sums of the segment;
//             the bytes into the segment's own staging area.
//   assemble  one workgroup per frame: prefix sum of the segment sizes, the combined checksums, the capacity check, the
//             file's head and tail, nbytes and status.
//   place     one workgroup per segment: the staging area into the slot, in dwords aligned on the SLOT (the source is read as
//             two aligned dwords and shifted), bytes only at either end.
#include "common.h"
#include "png_enc_device.h"

namespace pr {
namespace {

using namespace pngenc;

constexpr int kFrameThreads = 256;

struct EncWave64 {
  static constexpr int L = 64;
  __device__ __forceinline__ int lane() const { return (int)threadIdx.x; }
  __device__ __forceinline__ void sync() const { __syncthreads(); }
  __device__ __forceinline__ uint64_t ballot(bool b) const { return __ballot(b); }
  __device__ __forceinline__ uint32_t scan_add(uint32_t v) const {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const uint32_t t = (uint32_t)__shfl_up((int)v, d, 64);
      if ((int)threadIdx.x >= d) v += t;
    }
    return v;
  }
  __device__ __forceinline__ uint32_t reduce_add(uint32_t v) const {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += (uint32_t)__shfl_xor((int)v, d, 64);
    return v;
  }
  __device__ __forceinline__ uint32_t reduce_xor(uint32_t v) const {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v ^= (uint32_t)__shfl_xor((int)v, d, 64);
    return v;
  }
  __device__ __forceinline__ uint32_t last(uint32_t v) const { return (uint32_t)__shfl((int)v, 63, 64); }
  __device__ __forceinline__ void or_word(uint32_t* p, uint32_t v) const { atomicOr(p, v); }
  __device__ __forceinline__ void add_word(uint32_t* p, uint32_t v) const { atomicAdd(p, v); }
};

struct EncParams {
  pr_png_enc_args a;
  int nseg, fixed, rowf_stride;
  int64_t raw;
  uint8_t* stage;      // [F][nseg][kStage]
  SegRec* rec;         // [F][nseg]
  int32_t* seg_off;    // [F][nseg]  the segment's offset behind the file's head
  uint8_t* rowf;       // [F][rowf_stride]
  int32_t* fstate;     // [F]        1 = the frame does not fit its slot
};

__device__ __forceinline__ FilterSrc frame_source(const EncParams& p, int f) {
  FilterSrc s;
  s.frame = p.a.frames + (int64_t)f * p.a.H * p.a.W * 3;
  s.H = p.a.H, s.W = p.a.W, s.bgr = p.a.bgr, s.fixed = p.fixed;
  s.rowf = p.rowf + (int64_t)f * p.rowf_stride;
  return s;
}

__global__ void __launch_bounds__(64) png_enc_choose_kernel(EncParams p) {
  const int row = (int)blockIdx.x, f = (int)blockIdx.y;
  const EncWave64 w;
  const int t = choose_row(w, frame_source(p, f), row);
  if (threadIdx.x == 0) p.rowf[(int64_t)f * p.rowf_stride + row] = (uint8_t)t;
}

__global__ void __launch_bounds__(64) png_enc_segment_kernel(EncParams p) {
  __shared__ SegScratch<64> scratch;
  const int s = (int)blockIdx.x, f = (int)blockIdx.y;
  const int64_t begin = (int64_t)s * kSeg;
  const int n = (int)min((int64_t)kSeg, p.raw - begin);
  const int64_t fs = (int64_t)f * p.nseg + s;
  const EncWave64 w;
  encode_segment(w, scratch, frame_source(p, f), begin, n, s == p.nseg - 1, p.a.mode, p.a.plan->crc_pow, p.stage + fs * kStage,
                 p.rec + fs);
}

__global__ void __launch_bounds__(kFrameThreads) png_enc_assemble_kernel(EncParams p) {
  __shared__ uint32_t sh_off[kFrameThreads], sh_crc[kFrameThreads], sh_a[kFrameThreads], sh_b[kFrameThreads];
  __shared__ uint32_t sh_total;
  const int f = (int)blockIdx.x, t = (int)threadIdx.x;
  const pr_png_enc_plan& plan = *p.a.plan;
  const SegRec* rec = p.rec + (int64_t)f * p.nseg;
  int32_t* seg_off = p.seg_off + (int64_t)f * p.nseg;
  const int per = (p.nseg + kFrameThreads - 1) / kFrameThreads;
  const int s0 = min(t * per, p.nseg), s1 = min(s0 + per, p.nseg);
  uint32_t sum = 0;
  for (int s = s0; s < s1; ++s) sum += rec[s].len;
  sh_off[t] = sum;
  __syncthreads();
  if (t == 0) {
    uint32_t at = 0;
    for (int i = 0; i < kFrameThreads; ++i) {
      const uint32_t here = sh_off[i];
      sh_off[i] = at;
      at += here;
    }
    sh_total = at;
  }
  __syncthreads();
  const uint32_t coded = sh_total;
  uint32_t off = sh_off[t];
  FrameSums sums;
  for (int s = s0; s < s1; ++s) {
    const SegRec r = rec[s];
    seg_off[s] = (int32_t)off;
    off += r.len;
    const int64_t end = min((int64_t)(s + 1) * kSeg, p.raw);
    add_segment(sums, r, coded - off, (uint64_t)(p.raw - end), plan.crc_pow);
  }
  sh_crc[t] = sums.crc_terms, sh_a[t] = sums.a, sh_b[t] = sums.b;
  __syncthreads();
  if (t != 0) return;
  for (int i = 1; i < kFrameThreads; ++i) {
    sums.crc_terms ^= sh_crc[i];
    sums.a = (sums.a + sh_a[i]) % kAdler;
    sums.b = (sums.b + sh_b[i]) % kAdler;
  }
  const int64_t size = (int64_t)PR_PNG_ENC_HEAD_BYTES + coded + 8 + PR_PNG_ENC_TAIL_BYTES;
  if (size > p.a.capacity) {
    p.a.nbytes[f] = 0;
    p.a.status[f] = (int)PR_PNG_ENC_ST_OVERFLOW;
    p.fstate[f] = 1;
    return;
  }
  p.a.nbytes[f] = (int32_t)size;
  p.a.status[f] = 0;
  p.fstate[f] = 0;
  const uint32_t adler = frame_adler(sums, (uint64_t)p.raw);
  const uint32_t crc = frame_idat_crc(sums, plan.idat_crc_head, coded, adler, plan.crc_pow);
  uint8_t* o = p.a.out + (int64_t)f * p.a.capacity;
  const uint32_t idat_len = 2u + coded + 4u;
  for (int i = 0; i < PR_PNG_ENC_HEAD_BYTES; ++i) o[i] = (i >= 33 && i < 37) ? (uint8_t)(idat_len >> (24 - 8 * (i - 33))) : plan.head[i];
  o += PR_PNG_ENC_HEAD_BYTES + coded;
  for (int k = 0; k < 4; ++k) o[k] = (uint8_t)(adler >> (24 - 8 * k));
  for (int k = 0; k < 4; ++k) o[4 + k] = (uint8_t)(crc >> (24 - 8 * k));
  for (int i = 0; i < PR_PNG_ENC_TAIL_BYTES; ++i) o[8 + i] = plan.tail[i];
}

__global__ void __launch_bounds__(kFrameThreads) png_enc_place_kernel(EncParams p) {
  const int s = (int)blockIdx.x, f = (int)blockIdx.y, t = (int)threadIdx.x;
  if (p.fstate[f]) return;
  const int64_t fs = (int64_t)f * p.nseg + s;
  const int len = (int)p.rec[fs].len;   // at most 5 + kSeg: whole dwords of the staging area reach to kStage at most
  const uint8_t* src = p.stage + fs * kStage;
  const uint32_t* sw = (const uint32_t*)src;
  uint8_t* dst = p.a.out + (int64_t)f * p.a.capacity + PR_PNG_ENC_HEAD_BYTES + p.seg_off[fs];
  const int head = min(len, (int)((4 - ((uintptr_t)dst & 3)) & 3));
  const int words = (len - head) / 4;
  if (t < head) dst[t] = src[t];
  uint32_t* dw = (uint32_t*)(dst + head);
  const int sh = 8 * (head & 3);
  for (int i = t; i < words; i += kFrameThreads) {   // destination word i = source bytes head + 4 i .. + 3 (head < 4)
    const uint32_t lo = sw[i];
    dw[i] = sh ? (lo >> sh) | (sw[i + 1] << (32 - sh)) : lo;
  }
  const int tail = head + 4 * words;
  if (t < len - tail) dst[tail + t] = src[tail + t];
}

}  // namespace
}  // namespace pr

extern "C" int pr_png_encode(const pr_png_enc_args* a, void* workspace, size_t workspace_bytes, void* stream) {
  using namespace pr;
  PR_REQUIRE(a, "pr_png_encode: null argument struct");
  PR_REQUIRE(a->F >= 0, "pr_png_encode: F = %d", a->F);
  if (a->F == 0) return PR_OK;
  EncLayout l;
  PR_REQUIRE(enc_layout(a->F, a->H, a->W, &l), "pr_png_encode: %d frames of %d x %d: at most 65535 frames, sizes 1..%d", a->F, a->W, a->H,
             PR_PNG_MAX_SIDE);
  PR_REQUIRE(a->filter >= 0 && a->filter <= PR_PNG_ENC_FILTER_ADAPTIVE, "pr_png_encode: filter %d is not 0..4 or 5 (adaptive)", a->filter);
  PR_REQUIRE(a->mode == PR_PNG_ENC_STORED || a->mode == PR_PNG_ENC_RLE, "pr_png_encode: mode %d is neither PR_PNG_ENC_STORED nor PR_PNG_ENC_RLE",
             a->mode);
  PR_REQUIRE(a->capacity >= 0 && a->capacity <= 0x7fffffffl, "pr_png_encode: capacity %lld is outside 0..2^31-1", (long long)a->capacity);
  PR_REQUIRE(a->frames, "pr_png_encode: null frames");
  PR_REQUIRE(a->plan, "pr_png_encode: null plan");
  PR_REQUIRE(a->out || a->capacity == 0, "pr_png_encode: null out");
  PR_REQUIRE(a->nbytes, "pr_png_encode: null nbytes");
  PR_REQUIRE(a->status, "pr_png_encode: null status");
  PR_REQUIRE(workspace, "pr_png_encode: null workspace");
  PR_REQUIRE(((uintptr_t)workspace & 15) == 0, "pr_png_encode: workspace is not 16-byte aligned");
  PR_REQUIRE(workspace_bytes >= l.total, "pr_png_encode: workspace of %zu bytes, %zu needed for %d frames of %d x %d", workspace_bytes,
             l.total, a->F, a->W, a->H);
  EncParams p;
  p.a = *a;
  p.nseg = l.nseg;
  p.raw = l.raw;
  p.fixed = a->mode == PR_PNG_ENC_STORED ? 0 : a->filter;
  p.rowf_stride = l.rowf_stride;
  char* ws = (char*)workspace;
  p.stage = (uint8_t*)(ws + l.stage);
  p.rec = (SegRec*)(ws + l.rec);
  p.seg_off = (int32_t*)(ws + l.seg_off);
  p.rowf = (uint8_t*)(ws + l.rowf);
  p.fstate = (int32_t*)(ws + l.fstate);
  hipStream_t s = (hipStream_t)stream;
  const unsigned F = (unsigned)a->F;
  if (p.fixed == PR_PNG_ENC_FILTER_ADAPTIVE) {
    hipLaunchKernelGGL(png_enc_choose_kernel, dim3((unsigned)a->H, F), dim3(64), 0, s, p);
    PR_TRY(check_launch("png_enc_choose_kernel"));
  }
  hipLaunchKernelGGL(png_enc_segment_kernel, dim3((unsigned)l.nseg, F), dim3(64), 0, s, p);
  PR_TRY(check_launch("png_enc_segment_kernel"));
  hipLaunchKernelGGL(png_enc_assemble_kernel, dim3(F), dim3(kFrameThreads), 0, s, p);
  PR_TRY(check_launch("png_enc_assemble_kernel"));
  hipLaunchKernelGGL(png_enc_place_kernel, dim3((unsigned)l.nseg, F), dim3(kFrameThreads), 0, s, p);
  return check_launch("png_enc_place_kernel");
}
