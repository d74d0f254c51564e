// Annotated score video (ABI 15): every canvas of <TITLE>_video -- the source frame with the track's box, area-resampled to
// dst_w x dst_h, beside a text panel -- composed in one launch.  The contract (box, integer-exact area resample, panel text)
// is written in include/poserisk_hip.h above pr_compose_video; tests/video_ref.py restates it in numpy and
// tests/test_video_gpu.py compares every byte.
//
// One workgroup owns a band of R destination rows of one canvas.  By its bytes the kernel should be HBM-bound (3 H W in,
// 3 dst_h (dst_w + panel_w) out per canvas) and both directions move 16 bytes per lane; measured, it is bound by the latency
// of the horizontal pass under the occupancy LDS allows (11 % of the byte floor at 800x450).
//   phase A  vertical pass.  A thread owns 16 consecutive bytes of the source rows (a byte is one channel of one pixel, so
//            the 3-byte interleave needs no shuffling on this axis), loads them from each of the few source rows a destination
//            row overlaps, paints the box, and sums them with the row weights oy into V[r][3 x + c] (u32, <= 255 H) in LDS.
//   phase B  horizontal pass.  The band of the canvas is one contiguous byte range of `out`; a thread owns 16-byte-aligned
//            pieces of it.  A piece inside the image region: branch-free, the tap count a template argument, 16 x T reads of V
//            issued together, sum of ox V, the rounded division, one 16-byte store.  A panel piece no line of this band
//            reaches: zeros.  Pieces with text, across the image's edge, a row's end or the band's ragged ends: byte by byte
//            (the bytes of a piece that belong to a neighbouring band are that band's).
// The only LDS traffic of weight is V: phase A writes 16 consecutive dwords per lane (four ds_write_b128 at a lane stride of 64
// bytes), phase B gathers 2 - 4 taps per output byte at a lane stride of about 18 dwords; both shapes conflict across banks.
#include "common.h"

// the workgroup's dynamic LDS block: V, the first-tap table, the line table (at file scope so that a host build can supply it)
extern __shared__ __attribute__((aligned(16))) unsigned pr_compose_lds[];

namespace pr {
namespace {

constexpr int kThreads = 256;
constexpr int kMaxRows = 8;               // destination rows per band at most
// Bytes of LDS for V: R = kVBudget / (4 * pitch), 1 <= R <= kMaxRows.  Measured at 64 x 800x450 (scripts/bench_video.py): 64 KB
// (R = 6, 2 workgroups a CU) 0.54 ms, 48 KB (R = 5, 3 a CU) 0.37 ms, 32 KB (R = 3, 5 a CU) 0.25 ms, 20 KB (R = 2, 7 a CU) 0.27 ms:
// the kernel lives on the waves in flight, until the bands get so thin that their shared source rows are read too often.
constexpr int kVBudget = 32 * 1024;
constexpr int kMaxLines = PR_VIDEO_MAX_LINES;
constexpr int kFar = 1 << 22;               // farther than any box edge or line origin that can touch a canvas
constexpr int kLineWords = 6;              // x0, canvas row of atlas row 0, size class, length, colour, advance

struct Params {
  pr_compose_args a;
  int R, nbands, pitch;   // pitch: dwords per V row (3 W rounded up to 16)
  int xk_words;           // dwords of the first-tap table (dst_w u16, rounded up to 16 bytes)
  unsigned box_rgb;       // channel c in bits 8 c .. 8 c + 7
};

__device__ __forceinline__ unsigned div3(unsigned v) { return (v * 43691u) >> 17; }   // exact below 65536

// S / D rounded half to even, S <= 255 D, D <= 2^24: a float estimate of the quotient is within one of it, the remainder
// (taken mod 2^32, |r| < 2^25) corrects it.
__device__ __forceinline__ unsigned round_div(unsigned S, unsigned D, float invD) {
  unsigned q = (unsigned)(__uint2float_rn(S) * invD);
  int r = (int)(S - q * D);
  if (r < 0) { --q; r += (int)D; }
  else if (r >= (int)D) { ++q; r -= (int)D; }
  const unsigned r2 = 2u * (unsigned)r;
  if (r2 > D || (r2 == D && (q & 1u))) ++q;
  return q;
}

__device__ __forceinline__ bool on_box(int x, bool row_outer, bool row_inner, int bx0, int bx1) {
  // outline +-1 (Chebyshev): inside [x_min-1, x_max+1] x [y_min-1, y_max+1], not inside [x_min+2, x_max-2] x [y_min+2, y_max-2]
  return row_outer && x >= bx0 - 1 && x <= bx1 + 1 && !(row_inner && x >= bx0 + 2 && x <= bx1 - 2);
}

// T: the most source columns a destination column overlaps (its taps), 1 .. 4, or 0 for more: then every image byte takes the
// byte-by-byte path.
template <int T>
__global__ void __launch_bounds__(kThreads) compose_kernel(Params p) {
  unsigned* lds = pr_compose_lds;
  const pr_compose_args& a = p.a;
  unsigned* V = lds;                                               // [R][pitch]
  unsigned short* xk = (unsigned short*)(lds + p.R * p.pitch);     // [dst_w] first source column of destination column i
  int (*line_s)[kLineWords] = (int (*)[kLineWords])(lds + p.R * p.pitch + p.xk_words);   // [kMaxLines] lines of this canvas
  unsigned& line_mask = lds[p.R * p.pitch + p.xk_words + kMaxLines * kLineWords];        // the lines that reach this band

  const int n = blockIdx.x / p.nbands, band = blockIdx.x - n * p.nbands;
  const int r0 = band * p.R, rows = min(p.R, a.dst_h - r0);
  const int tid = threadIdx.x;
  const int W3 = 3 * a.W;
  const int fi = a.src_idx ? a.src_idx[n] : n;
  const bool have = (unsigned)fi < (unsigned)a.n_frames;
  if (band == 0 && tid == 0 && a.status) a.status[n] = have ? 0 : 1;

  // ---- tables: first tap per destination column, the lines that reach this band -------------------------------------
  for (int i = tid; i < a.dst_w; i += kThreads) xk[i] = (unsigned short)((unsigned)(i * a.W) / (unsigned)a.dst_w);
  if (tid == 0) line_mask = 0u;
  __syncthreads();
  if (tid < a.L) {
    const int* ln = a.lines + ((long)n * a.L + tid) * PR_VIDEO_LINE_INTS;
    const int cls = ln[2], len = min(ln[3], a.C);
    bool live = (unsigned)cls < (unsigned)a.S && len > 0;
    int adv = 1, ascent = 0;
#pragma unroll
    for (int s = 0; s < PR_VIDEO_MAX_CLASSES; ++s)
      if (cls == s) { adv = a.adv[s]; ascent = a.ascent[s]; }
    // origins are any int32: beyond +-kFar a line cannot reach a canvas of <= 8192 x 4096 pixels with cells of <= 256 rows and
    // <= 4096 * 256 columns, so clamping changes nothing and keeps the differences below inside int32
    const int x0 = min(max(ln[0], -kFar), kFar);
    const int top = min(max(ln[1], -kFar), kFar) - ascent;
    line_s[tid][0] = x0; line_s[tid][1] = top; line_s[tid][2] = cls;
    line_s[tid][3] = len;   line_s[tid][4] = ln[4]; line_s[tid][5] = adv;
    live = live && top < r0 + rows && top + a.CH > r0;
    if (live) atomicOr(&line_mask, 1u << tid);
  }

  // ---- phase A: V[r][xc] = sum_j oy[r][j] boxed_src[j][xc] ---------------------------------------------------------------
  const int npieces = p.pitch >> 4;
  int bx0 = 0, bx1 = -1, by0 = 0, by1 = 0;
  if (a.box) {
    const int* b = a.box + (long)n * 4;
    bx0 = b[0]; by0 = b[1]; bx1 = b[2]; by1 = b[3];
  }
  const bool has_box = bx1 >= bx0;
  // corners are any int32: clamped (after the x_max < x_min test) to where they are off every frame anyway, so that the +-1
  // and +-2 below stay inside int32
  bx0 = min(max(bx0, -kFar), kFar); bx1 = min(max(bx1, -kFar), kFar);
  by0 = min(max(by0, -kFar), kFar); by1 = min(max(by1, -kFar), kFar);
  const uint8_t* frame = a.frames + (long)(have ? fi : 0) * a.H * W3;
  for (int item = tid; item < rows * npieces; item += kThreads) {
    const int r = item / npieces, piece = item - r * npieces;
    const int xc0 = piece << 4, nvalid = min(16, W3 - xc0);
    unsigned acc[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) acc[q] = 0u;
    if (have) {
      const int y = r0 + r;
      const int lo = y * a.H, hi = lo + a.H;                       // this destination row in units of 1 / (H dst_h)
      const unsigned px0 = div3((unsigned)xc0);                    // pixel and channel of the piece's first byte
      const int ch0 = xc0 - 3 * (int)px0;
      for (int j = lo / a.dst_h; j * a.dst_h < hi; ++j) {
        const unsigned oy = (unsigned)(min((j + 1) * a.dst_h, hi) - max(j * a.dst_h, lo));
        const uint8_t* src = frame + (long)j * W3 + xc0;
        uint8_t b[16];
        if (nvalid == 16) {
          __builtin_memcpy(b, src, 16);                            // one 16-byte load (rows need not be 16-byte aligned)
        } else {
#pragma unroll
          for (int q = 0; q < 16; ++q) b[q] = q < nvalid ? src[q] : (uint8_t)0;
        }
        const bool row_outer = has_box && j >= by0 - 1 && j <= by1 + 1;
        const bool row_inner = j >= by0 + 2 && j <= by1 - 2;
        // the piece spans pixels px0 .. px0 + 5: skip the per-byte test where the row or the span cannot touch the box
        if (row_outer && (int)px0 <= bx1 + 1 && (int)px0 + 5 >= bx0 - 1) {
          int x = (int)px0, c = ch0;
#pragma unroll
          for (int q = 0; q < 16; ++q) {
            if (on_box(x, row_outer, row_inner, bx0, bx1)) b[q] = (uint8_t)(p.box_rgb >> (8 * c));
            if (++c == 3) { c = 0; ++x; }
          }
        }
#pragma unroll
        for (int q = 0; q < 16; ++q) acc[q] += oy * (unsigned)b[q];
      }
    }
    uint4* dst = (uint4*)(V + r * p.pitch + xc0);
#pragma unroll
    for (int q = 0; q < 4; ++q) dst[q] = make_uint4(acc[4 * q], acc[4 * q + 1], acc[4 * q + 2], acc[4 * q + 3]);
  }
  __syncthreads();

  // ---- phase B: the band's bytes of `out`, 16 aligned bytes per thread ---------------------------------------------------
  const int rowbytes = 3 * (a.dst_w + a.panel_w), img_bytes = 3 * a.dst_w;
  const unsigned D = (unsigned)a.H * (unsigned)a.W;
  const float invD = 1.0f / (float)D;
  const unsigned mask = line_mask;
  uint8_t* band_out = a.out + ((size_t)n * a.dst_h + r0) * rowbytes;
  const int nbytes = rows * rowbytes;
  const int lead = (int)((uintptr_t)band_out & 15);                // bytes of the first piece that lie in front of the band
  const int npc = (lead + nbytes + 15) >> 4;
  for (int pc = tid; pc < npc; pc += kThreads) {
    const int off0 = (pc << 4) - lead;                             // band byte offset of the piece's first byte (may be < 0)
    uint8_t* P = band_out + off0;                                  // 16-byte aligned
    const int first = off0 < 0 ? 0 : off0;
    const int r = first / rowbytes, col = first - r * rowbytes;
    const bool whole = off0 >= 0 && off0 + 16 <= nbytes && col + 16 <= rowbytes;   // 16 bytes of one row of this band
    if (T > 0 && whole && col + 16 <= img_bytes) {
      // image: every byte on its own and branch-free, so that the 16 table reads and the 16 T taps issue together
      const unsigned* vrow = V + r * p.pitch;
      unsigned w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const unsigned i = div3((unsigned)(col + q));
        const int c = col + q - 3 * (int)i;
        const int lo = (int)i * a.W, hi = lo + a.W;                // this destination column in units of 1 / (W dst_w)
        const int k0 = xk[i];
        unsigned S = 0u;                                           // <= 255 H W < 2^32 for H, W <= 4096: u32 is exact
#pragma unroll
        for (int t = 0; t < (T > 0 ? T : 1); ++t) {
          const int s0 = (k0 + t) * a.dst_w;                       // a tap past the column's last has weight 0
          const int wt = max(min(s0 + a.dst_w, hi) - max(s0, lo), 0);
          S += (unsigned)wt * vrow[3 * min(k0 + t, a.W - 1) + c];
        }
        w[q >> 2] |= round_div(S, D, invD) << (8 * (q & 3));
      }
      *(uint4*)__builtin_assume_aligned(P, 16) = make_uint4(w[0], w[1], w[2], w[3]);
      continue;
    }
    if (whole && col >= img_bytes) {
      // panel: black unless one of this band's lines reaches the piece's pixels
      const int xa = (int)div3((unsigned)col), xb = (int)div3((unsigned)(col + 15));
      bool hit = false;
      for (unsigned m = mask; m; m &= m - 1u) {
        const int* ln = line_s[__builtin_ctz(m)];
        hit = hit || (xb >= ln[0] && xa < ln[0] + ln[3] * ln[5]);
      }
      if (!hit) {
        *(uint4*)__builtin_assume_aligned(P, 16) = make_uint4(0u, 0u, 0u, 0u);
        continue;
      }
    }
    // everything else -- pieces with text, pieces across the image's edge, a row's end or the band's ends -- byte by byte
    int rr = r, cc = col;
#pragma unroll 1
    for (int q = first - off0; q < 16 && off0 + q < nbytes; ++q) {
      unsigned val = 0u;
      if (cc < img_bytes) {
        const unsigned i = div3((unsigned)cc);
        const int c = cc - 3 * (int)i;
        const int lo = (int)i * a.W, hi = lo + a.W;
        const unsigned* vr = V + rr * p.pitch + c;
        int k = xk[i];
        unsigned S = 0u;
        for (int s0 = k * a.dst_w; s0 < hi; s0 += a.dst_w, ++k)
          S += (unsigned)(min(s0 + a.dst_w, hi) - max(s0, lo)) * vr[3 * k];
        val = round_div(S, D, invD);
      } else {
        const unsigned px = div3((unsigned)cc);
        const int c = cc - 3 * (int)px, x = (int)px, y = r0 + rr;
        for (unsigned m = mask; m; m &= m - 1u) {
          const int* ln = line_s[__builtin_ctz(m)];
          const int cls = ln[2], adv = ln[5];
          const int v = y - ln[1], dx = x - ln[0];
          if (v < 0 || v >= a.CH || dx < 0 || dx >= ln[3] * adv) continue;
          const int k = dx / adv, u = dx - k * adv;
          const int code = a.text[((long)n * a.L + __builtin_ctz(m)) * a.C + k];
          if (code < 32 || code > 127) continue;
          const unsigned cov = a.atlas[(((long)cls * 96 + (code - 32)) * a.CH + v) * a.CW + u];
          const unsigned colr = (unsigned)((ln[4] >> (8 * c)) & 255);
          val = (2u * (val * (255u - cov) + colr * cov) + 255u) / 510u;
        }
      }
      P[q] = (uint8_t)val;
      if (++cc == rowbytes) { cc = 0; ++rr; }
    }
  }
}

}  // namespace
}  // namespace pr

extern "C" int pr_compose_video(const pr_compose_args* a, void* stream) {
  using namespace pr;
  PR_REQUIRE(a, "pr_compose_video: null argument struct");
  PR_REQUIRE(a->N >= 0, "pr_compose_video: N = %d", a->N);
  if (a->N == 0) return PR_OK;
  PR_REQUIRE(a->out, "pr_compose_video: null out");
  PR_REQUIRE(a->frames, "pr_compose_video: null frames");
  PR_REQUIRE(a->n_frames >= 1, "pr_compose_video: n_frames = %d", a->n_frames);
  PR_REQUIRE(a->H >= 1 && a->W >= 1 && a->H <= 4096 && a->W <= 4096, "pr_compose_video: frame H x W = %d x %d outside 1..4096",
             a->H, a->W);
  PR_REQUIRE(a->dst_w >= 1 && a->dst_w <= 4096, "pr_compose_video: dst_w = %d outside 1..4096", a->dst_w);
  PR_REQUIRE(a->dst_h >= 1 && a->dst_h <= 4096, "pr_compose_video: dst_h = %d outside 1..4096", a->dst_h);
  PR_REQUIRE(a->panel_w >= 0 && a->panel_w <= 4096, "pr_compose_video: panel_w = %d outside 0..4096", a->panel_w);
  PR_REQUIRE(a->L >= 0 && a->L <= PR_VIDEO_MAX_LINES, "pr_compose_video: L = %d lines outside 0..%d", a->L, PR_VIDEO_MAX_LINES);
  if (a->L > 0) {
    PR_REQUIRE(a->lines && a->text && a->atlas, "pr_compose_video: null lines, text or atlas with L = %d", a->L);
    PR_REQUIRE(a->C >= 1 && a->C <= 4096, "pr_compose_video: C = %d codes per line outside 1..4096", a->C);
    PR_REQUIRE(a->S >= 1 && a->S <= PR_VIDEO_MAX_CLASSES, "pr_compose_video: S = %d size classes outside 1..%d", a->S,
               PR_VIDEO_MAX_CLASSES);
    PR_REQUIRE(a->CH >= 1 && a->CW >= 1 && a->CH <= 256 && a->CW <= 256, "pr_compose_video: atlas cell CH x CW = %d x %d outside 1..256",
               a->CH, a->CW);
    for (int s = 0; s < a->S; ++s) {
      PR_REQUIRE(a->adv[s] >= 1 && a->adv[s] <= a->CW, "pr_compose_video: adv[%d] = %d outside 1..CW = %d", s, a->adv[s], a->CW);
      PR_REQUIRE(a->ascent[s] >= -4096 && a->ascent[s] <= 4096, "pr_compose_video: ascent[%d] = %d", s, a->ascent[s]);
    }
  }
  PR_REQUIRE(a->src_idx || a->N <= a->n_frames, "pr_compose_video: %d canvases for %d frames without src_idx", a->N, a->n_frames);
  Params p;
  p.a = *a;
  p.box_rgb = (unsigned)a->box_rgb[0] | (unsigned)a->box_rgb[1] << 8 | (unsigned)a->box_rgb[2] << 16;
  p.pitch = (3 * a->W + 15) & ~15;
  p.R = std::min(kMaxRows, std::max(1, kVBudget / (4 * p.pitch)));
  p.R = std::min(p.R, a->dst_h);
  p.nbands = (a->dst_h + p.R - 1) / p.R;
  PR_REQUIRE((long)a->N * p.nbands < (1l << 31), "pr_compose_video: batch too large (N = %d)", a->N);
  p.xk_words = ((a->dst_w * 2 + 15) & ~15) / 4;
  const size_t lds = ((size_t)p.R * p.pitch + p.xk_words + kMaxLines * kLineWords + 4) * 4;   // <= 48 KB (one row of W = 4096) + 8 KB + 400 B
  int taps = 0;
  for (long i = 0; i < a->dst_w; ++i)
    taps = std::max(taps, (int)(((i + 1) * a->W + a->dst_w - 1) / a->dst_w - i * a->W / a->dst_w));
  const dim3 grid((unsigned)((long)a->N * p.nbands)), block(kThreads);
  hipStream_t s = (hipStream_t)stream;
  switch (taps) {
    case 1: hipLaunchKernelGGL(compose_kernel<1>, grid, block, lds, s, p); break;
    case 2: hipLaunchKernelGGL(compose_kernel<2>, grid, block, lds, s, p); break;
    case 3: hipLaunchKernelGGL(compose_kernel<3>, grid, block, lds, s, p); break;
    case 4: hipLaunchKernelGGL(compose_kernel<4>, grid, block, lds, s, p); break;
    default: hipLaunchKernelGGL(compose_kernel<0>, grid, block, lds, s, p); break;
  }
  return check_launch("compose_kernel");
}
