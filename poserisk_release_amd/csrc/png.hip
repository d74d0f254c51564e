// Device half of the PNG decoder: everything behind the chunk walk of csrc/png_host.cc.  The contract -- what is accepted, the
// inflate rule, what a bad stream may and may not do -- is written in include/poserisk_hip.h, section j4; the decoding text
// itself is csrc/png_device.h, instantiated here with 64 lanes and by tests/native/png_native.cc with one lane on the host
// under sanitizers; tests/png_ref.py restates it in Python and tests/test_png_gpu.py compares every byte with Pillow's.
//
//   gather    a workgroup per frame: the IDAT payloads, 256 ranges at a time (lengths scanned in LDS), are copied into one
//             contiguous zlib stream in the frame's part of the workspace, which starts at the first range's own offset so that
//             source and destination share their phase: 16 bytes a lane where they do mod 16, a dword a lane where they do mod
//             4 (twelve bytes of chunk overhead lie between two ranges), a byte a lane otherwise.  The bit reader then never
//             sees a chunk boundary.
//   inflate   ONE WAVE per frame, four frames a workgroup (4 x 4.1 KB of tables and 4.1 KB of fixed tables in LDS: 20.5 KB, so
//             seven workgroups fit a CU's 160 KB).  The bit buffer and the symbol decode are wave-uniform; the 64 lanes
//             build a dynamic block's tables together, store batches of up to 64 literals with one instruction and copy
//             every match together.  A frame is one serial chain of symbols: the kernel's rate comes from the number of
//             frames in flight, as pr_jpeg_decode's does.
//   unfilter  a workgroup per frame: Adler-32 of the inflated bytes by all 256 lanes, the filters undone in place as a skewed
//             wavefront (lane l one pixel behind lane l - 1, 64 rows a pass, passes that start on a None / Sub row side by
//             side on the workgroup's waves), then colour conversion by all lanes, twelve bytes a lane.
#include "common.h"
#include "png_device.h"

namespace pr {
namespace png {
namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;

struct PngMeta {   // one per frame, in the workspace
  uint32_t adler;  // the trailer's Adler-32, written by the inflate kernel when it ends with status 0
  uint32_t pad[3];
};

struct PngParams {
  pr_png_args a;
  uint8_t* streams;      // the gathered zlib streams: frame f's at stream_offset(f)
  int64_t stream_cap;    // bytes of `streams`
  PngMeta* meta;
  uint8_t* raw;          // the inflated scanlines: frame f's at f * raw_stride
  int64_t raw_stride;    // H (1 + 4 W), padded to 16: room for every colour type
};

struct PngWave64 {
  static constexpr int L = 64;
  __device__ __forceinline__ int lane() const { return (int)(threadIdx.x & 63u); }
  __device__ __forceinline__ uint32_t uniform(uint32_t v) const { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
  __device__ __forceinline__ uint32_t read_lane(uint32_t v, int k) const {
    return (uint32_t)__builtin_amdgcn_readlane((int)v, __builtin_amdgcn_readfirstlane(k));
  }
  __device__ __forceinline__ uint64_t ballot(bool p) const { return __ballot(p); }
  __device__ __forceinline__ int rank(uint64_t m) const { return __builtin_popcountll(m & ((1ull << lane()) - 1ull)); }
  __device__ __forceinline__ uint32_t shfl_up1(uint32_t v) const { return (uint32_t)__shfl_up((int)v, 1); }
  // LDS: a wave's DS instructions execute in order, so a table entry another lane of this wave wrote is there once the
  // compiler keeps the accesses in program order; the fence does that and costs no instruction.
  __device__ __forceinline__ void table_sync() const {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
  }
  // A match reads bytes that OTHER lanes of this wave stored to global memory a few instructions earlier.  Loads and stores
  // are counted together in vmcnt but return out of order with respect to each other, and the compiler knows of no
  // dependence between one lane's store and another lane's load, so the order is made explicit: wait until every store of
  // the wave has been acknowledged, then fence.  The loads that follow go through this CU's own vector L1, which this wave's
  // stores went through too (a CU's L1 is never refreshed by ANOTHER CU's stores -- cdna_hip_programming.md section 6,
  // Guideline 16; MI355X_MICROARCH.md, inter-workgroup visibility -- but a frame's bytes are written and read by one wave
  // only, so no agent-scope acquire is needed).  inflate() calls this only when a match reaches into bytes stored since the
  // last call.
  __device__ __forceinline__ void stores_before_loads() const {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  }
  __device__ __forceinline__ uint32_t load_word(const uint8_t* z, int64_t off, int64_t) const {
    return *reinterpret_cast<const uint32_t*>(z + off);   // off is a multiple of 4 below len; the frame's slot is padded to 16
  }
};

__device__ __forceinline__ int64_t align16(int64_t n) { return (n + 15) & ~(int64_t)15; }

// Where frame f's gathered stream lies: at its first IDAT range's own offset in `data`, so that the first range's source and
// destination share their phase mod 16 (both buffers are 16-byte aligned) and no prefix over frames is needed.  Streams of
// different files cannot meet there: a stream is no longer than the rest of its file behind that offset, and files do not
// overlap.  The inflate kernel reads whole dwords, from the 16-byte line the slot starts in: stream_cap is data_bytes rounded
// up to 16 and 16 more.  false when the slot would leave the bytes the files occupy.
__device__ __forceinline__ bool stream_slot(const PngParams& p, const pr_png_frame& fr, int64_t* off) {
  const pr_png_idat first = p.a.idat[fr.first_idat];
  if (first.begin < 0 || first.begin > p.a.data_bytes) return false;
  *off = first.begin;
  return fr.zlib_bytes <= p.a.data_bytes - first.begin;
}

// 16-byte stores: the project's convention for the store-data hazard (csrc/kernel_vocab.h, README "hardware rules") -- the data
// registers stay live and unwritten for the wait states behind the store.
__device__ __forceinline__ void store_b128(uint4* dst, uint4 v) {
  *dst = v;
  asm volatile("s_nop 3" ::"v"(v.x), "v"(v.y), "v"(v.z), "v"(v.w) : "memory");
}

__global__ void __launch_bounds__(kThreads) png_gather_kernel(PngParams p) {
  __shared__ int64_t s_off[kThreads + 1];
  __shared__ int s_bad;
  const pr_png_args& a = p.a;
  const int f = (int)blockIdx.x, t = (int)threadIdx.x;
  const pr_png_frame fr = a.frames[f];
  int64_t slot = 0;
  if (!frame_ok(fr, a) || !stream_slot(p, fr, &slot)) {
    if (t == 0) atomicOr(a.status + f, (int)PR_PNG_ST_REFUSED);
    return;
  }
  uint8_t* dst0 = p.streams + slot;
  if (t == 0) s_bad = 0;
  int64_t done = 0;   // bytes gathered by the batches before this one
  for (int r0 = 0; r0 < fr.n_idat; r0 += kThreads) {
    const int n = min(kThreads, fr.n_idat - r0);
    __syncthreads();
    int64_t mine = 0;
    if (t < n) {
      const int i = fr.first_idat + r0 + t;
      const pr_png_idat g = a.idat[i];
      const int64_t prev_end = (r0 + t) > 0 ? a.idat[i - 1].end : 0;
      if (g.begin < prev_end || g.begin > g.end || g.end > a.data_bytes) atomicOr(&s_bad, 1);
      else mine = g.end - g.begin;
    }
    s_off[t + 1] = mine;
    if (t == 0) s_off[0] = 0;
    __syncthreads();
    for (int d = 1; d < kThreads; d <<= 1) {   // inclusive scan of the lengths: s_off[i + 1] = sum of ranges 0..i
      const int64_t v = s_off[t + 1] + (t >= d ? s_off[t + 1 - d] : 0);
      __syncthreads();
      s_off[t + 1] = v;
      __syncthreads();
    }
    if (s_bad || done + s_off[n] > fr.zlib_bytes) {   // a range outside the data, out of order, or more bytes than stated
      if (t == 0) atomicOr(a.status + f, (int)PR_PNG_ST_REFUSED);
      return;
    }
    for (int r = 0; r < n; ++r) {
      const int64_t len = s_off[r + 1] - s_off[r];
      if (len == 0) continue;
      const uint8_t* src = a.data + a.idat[fr.first_idat + r0 + r].begin;
      uint8_t* dst = dst0 + done + s_off[r];
      // In phase mod 16 (always the first range, then every IDAT chunk whose 12 bytes of overhead add up to a multiple of 16):
      // 16 bytes a lane.  In phase mod 4 (what those 12 bytes leave otherwise): a dword a lane.  Else a byte a lane.
      const unsigned phase = (unsigned)(((uintptr_t)src ^ (uintptr_t)dst) & 15);
      if (phase == 0 && len >= 32) {
        const int64_t head = (int64_t)((16 - ((uintptr_t)dst & 15)) & 15), nvec = (len - head) >> 4, tail = head + (nvec << 4);
        if (t < head) dst[t] = src[t];
        for (int64_t i = t; i < nvec; i += kThreads)
          store_b128(reinterpret_cast<uint4*>(dst + head) + i, reinterpret_cast<const uint4*>(src + head)[i]);
        if (tail + t < len) dst[tail + t] = src[tail + t];
      } else if ((phase & 3) == 0 && len >= 8) {
        const int64_t head = (int64_t)((4 - ((uintptr_t)dst & 3)) & 3), nw = (len - head) >> 2, tail = head + (nw << 2);
        if (t < head) dst[t] = src[t];
        for (int64_t i = t; i < nw; i += kThreads)
          reinterpret_cast<uint32_t*>(dst + head)[i] = reinterpret_cast<const uint32_t*>(src + head)[i];
        if (tail + t < len) dst[tail + t] = src[tail + t];
      } else {
        for (int64_t i = t; i < len; i += kThreads) dst[i] = src[i];
      }
    }
    done += s_off[n];
  }
  if (done != fr.zlib_bytes && t == 0) atomicOr(a.status + f, (int)PR_PNG_ST_REFUSED);
}

__global__ void __launch_bounds__(kThreads) png_inflate_kernel(PngParams p) {
  __shared__ Tables s_fixed;
  __shared__ Tables s_dyn[kWaves];
  const pr_png_args& a = p.a;
  const PngWave64 w;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));   // wave-uniform: the descriptor and the bit buffer stay scalar
  if (wave == 0) build_fixed(w, &s_fixed);   // once per workgroup
  __syncthreads();
  const int f = (int)blockIdx.x * kWaves + wave;
  if (f >= a.F) return;
  const pr_png_frame fr = a.frames[f];
  int64_t slot = 0;
  if (!frame_ok(fr, a) || !stream_slot(p, fr, &slot)) return;   // the gather kernel has reported it
  if (a.status[f] != 0) return;                                 // ranges the gather kernel refused
  const int64_t raw = (int64_t)a.H * (1 + (int64_t)a.W * fr.bpp);
  uint32_t adler = 0;
  const int st = inflate(w, p.streams + (slot & ~(int64_t)15), slot & 15, fr.zlib_bytes, p.raw + (int64_t)f * p.raw_stride, raw, &s_dyn[wave], &s_fixed, &adler,
                         (InflateStats*)nullptr);
  if (w.lane() == 0) {
    if (st) atomicOr(a.status + f, st);
    p.meta[f].adler = adler;
  }
}

__global__ void __launch_bounds__(kThreads) png_unfilter_kernel(PngParams p) {
  __shared__ unsigned long long s_sum[2];
  __shared__ int s_flag;
  const pr_png_args& a = p.a;
  const PngWave64 w;
  const int f = (int)blockIdx.x, t = (int)threadIdx.x, wave = t >> 6;
  const pr_png_frame fr = a.frames[f];
  uint8_t* out = a.out + (int64_t)f * a.H * a.W * 3;
  const int64_t npx = (int64_t)a.H * a.W;
  const bool aligned = ((uintptr_t)out & 3) == 0;
  const int st0 = a.status[f];
  if (st0 != 0 || !frame_ok(fr, a)) {   // refused, or the inflate failed: zero pixels
    if (aligned) {
      for (int64_t i = t; i < (npx * 3) >> 2; i += kThreads) reinterpret_cast<uint32_t*>(out)[i] = 0u;
      for (int64_t i = ((npx * 3) & ~(int64_t)3) + t; i < npx * 3; i += kThreads) out[i] = 0;
    } else {
      for (int64_t i = t; i < npx * 3; i += kThreads) out[i] = 0;
    }
    return;
  }
  const int bpp = fr.bpp;
  const int64_t stride = 1 + (int64_t)a.W * bpp, nraw = stride * a.H;
  uint8_t* raw = p.raw + (int64_t)f * p.raw_stride;
  if (t == 0) s_sum[0] = s_sum[1] = 0, s_flag = 0;
  __syncthreads();
  uint32_t s1, s2;
  adler_partial(raw, nraw, t, kThreads, &s1, &s2);
  atomicAdd(&s_sum[0], (unsigned long long)s1);
  atomicAdd(&s_sum[1], (unsigned long long)s2);
  __syncthreads();
  int st = adler_combine(s_sum[0], s_sum[1], nraw) != p.meta[f].adler ? (int)PR_PNG_ST_CHECKSUM : 0;
  // Passes of 64 rows.  A round runs the next pass on wave 0 and, on waves 1.., the passes behind it for as long as each
  // starts on a row that needs nothing of the row above; the barrier between rounds makes a pass's last row visible to
  // the next round's first lane.  Every wave computes the same schedule from the filter bytes, which no pass writes.
  const int npass = (a.H + 63) / 64;
  for (int done = 0; done < npass;) {
    int run = 1;
    while (run < kWaves && done + run < npass && row_independent(raw, stride, (done + run) * 64)) ++run;
    if (wave < run && unfilter_pass(w, raw, a.H, a.W, bpp, (done + wave) * 64)) s_flag = 1;   // every lane the same value
    done += run;
    __syncthreads();
  }
  if (s_flag) st |= (int)PR_PNG_ST_FILTER;
  if (st && t == 0) atomicOr(a.status + f, st);
  const uint8_t* pal = fr.color_type == 3 ? a.palettes + (int64_t)fr.palette * 768 : nullptr;
  for (int64_t q = t; q < (npx + 3) >> 2; q += kThreads) {   // four pixels, twelve bytes a lane
    const int64_t px0 = q * 4;
    const int n = (int)min((int64_t)4, npx - px0);
    alignas(4) uint8_t bytes[12];
    int y = (int)(px0 / a.W), x = (int)(px0 - (int64_t)y * a.W);
    for (int i = 0; i < n; ++i) {
      colour_pixel(fr.color_type, bpp, raw + y * stride + 1 + (int64_t)x * bpp, pal, a.bgr, bytes + 3 * i);
      if (++x == a.W) x = 0, ++y;
    }
    uint8_t* dst = out + px0 * 3;
    if (n == 4 && aligned) {
      __builtin_memcpy(__builtin_assume_aligned(dst, 4), bytes, 12);
    } else {
      for (int i = 0; i < 3 * n; ++i) dst[i] = bytes[i];
    }
  }
}

size_t raw_stride_of(int H, int W) { return ((size_t)H * (1 + 4 * (size_t)W) + 15) & ~(size_t)15; }
size_t stream_cap_of(int64_t data_bytes) { return (((size_t)data_bytes + 15) & ~(size_t)15) + 16; }

}  // namespace
}  // namespace png
}  // namespace pr

extern "C" size_t pr_png_workspace_bytes(int F, int H, int W, int64_t data_bytes) {
  if (F <= 0 || H <= 0 || W <= 0 || H > PR_PNG_MAX_SIDE || W > PR_PNG_MAX_SIDE || data_bytes < 0) return 0;
  return pr::png::stream_cap_of(data_bytes) + (size_t)F * sizeof(pr::png::PngMeta) + (size_t)F * pr::png::raw_stride_of(H, W);
}

extern "C" int pr_png_decode(const pr_png_args* a, void* workspace, size_t workspace_bytes, void* stream) {
  using namespace pr;
  using namespace pr::png;
  PR_REQUIRE(a, "pr_png_decode: null argument struct");
  PR_REQUIRE(a->F >= 0, "pr_png_decode: F = %d", a->F);
  if (a->F == 0) return PR_OK;
  PR_REQUIRE(a->H >= 1 && a->W >= 1 && a->H <= PR_PNG_MAX_SIDE && a->W <= PR_PNG_MAX_SIDE, "pr_png_decode: H x W = %d x %d outside 1..%d",
             a->H, a->W, PR_PNG_MAX_SIDE);
  PR_REQUIRE(a->frames, "pr_png_decode: null frames");
  PR_REQUIRE(a->out, "pr_png_decode: null out");
  PR_REQUIRE(a->status, "pr_png_decode: null status");
  PR_REQUIRE(a->n_idat >= 0 && a->n_palettes >= 0 && a->data_bytes >= 0,
             "pr_png_decode: negative count (n_idat %d, n_palettes %d, data_bytes %lld)", a->n_idat, a->n_palettes,
             (long long)a->data_bytes);
  PR_REQUIRE(a->n_idat == 0 || (a->idat && a->data && a->data_bytes > 0),
             "pr_png_decode: %d IDAT ranges need data and idat (null pointer or data_bytes = %lld)", a->n_idat, (long long)a->data_bytes);
  PR_REQUIRE(a->n_palettes == 0 || a->palettes, "pr_png_decode: %d palettes and a null palettes pointer", a->n_palettes);
  PR_REQUIRE(((uintptr_t)a->frames & 7) == 0 && ((uintptr_t)a->idat & 7) == 0, "pr_png_decode: frames or idat is not 8-byte aligned");
  PR_REQUIRE(workspace, "pr_png_decode: null workspace");
  PR_REQUIRE(((uintptr_t)workspace & 15) == 0, "pr_png_decode: workspace is not 16-byte aligned");
  const size_t need = pr_png_workspace_bytes(a->F, a->H, a->W, a->data_bytes);
  if (workspace_bytes < need) {
    set_error("pr_png_decode: workspace of %zu bytes, %zu needed for %d frames of %d x %d and %lld bytes of files", workspace_bytes, need,
              a->F, a->H, a->W, (long long)a->data_bytes);
    return PR_ERR_CAPACITY;
  }
  PngParams p;
  p.a = *a;
  p.streams = (uint8_t*)workspace;
  p.stream_cap = (int64_t)stream_cap_of(a->data_bytes);
  p.meta = (PngMeta*)(p.streams + p.stream_cap);
  p.raw = (uint8_t*)(p.meta + a->F);
  p.raw_stride = (int64_t)raw_stride_of(a->H, a->W);
  hipStream_t s = (hipStream_t)stream;
  PR_HIP(hipMemsetAsync(a->status, 0, (size_t)a->F * sizeof(int32_t), s));
  hipLaunchKernelGGL(png_gather_kernel, dim3((unsigned)a->F), dim3(kThreads), 0, s, p);
  PR_TRY(check_launch("png_gather_kernel"));
  hipLaunchKernelGGL(png_inflate_kernel, dim3((unsigned)ceil_div(a->F, kWaves)), dim3(kThreads), 0, s, p);
  PR_TRY(check_launch("png_inflate_kernel"));
  hipLaunchKernelGGL(png_unfilter_kernel, dim3((unsigned)a->F), dim3(kThreads), 0, s, p);
  return check_launch("png_unfilter_kernel");
}
