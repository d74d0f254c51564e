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
//
// csrc/compose_shared.h holds what this kernel and csrc/compose_people.hip (pr_compose_people) compute alike; its head says why
// three pieces of it are macros.
#include "common.h"
#include "compose_shared.h"

// the workgroup's dynamic LDS block: V, the first-tap table, the line table (at file scope so that a host build can supply it)
extern __shared__ __attribute__((aligned(16))) unsigned pr_compose_lds[];

namespace pr {
namespace {

using namespace compose;
constexpr int kMaxLines = PR_VIDEO_MAX_LINES;

struct Params {
  pr_compose_args a;
  int R, nbands, pitch;   // compose::Band's
  int xk_words;
  unsigned box_rgb;       // channel c in bits 8 c .. 8 c + 7
};

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
    bool live;
    PR_COMPOSE_LOAD_LINE(a, n, tid, line_s[tid], r0, rows, live)
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
        load_piece(b, src, nvalid);
        PR_COMPOSE_PAINT_BOX(b, j, px0, ch0, has_box, bx0, by0, bx1, by1, p.box_rgb)
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
      const unsigned* vrow = V + r * p.pitch;
      PR_COMPOSE_IMAGE_PIECE((T > 0 ? T : 1), a, vrow, xk, col, D, invD, P)
      continue;
    }
    if (whole && col >= img_bytes) {
      // panel: black unless one of this band's lines reaches the piece's pixels
      const int xa = (int)div3((unsigned)col), xb = (int)div3((unsigned)(col + 15));
      const bool hit = lines_reach(mask, line_s, xa, xb);
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
        val = image_byte(a, V + rr * p.pitch, xk, cc, D, invD);
      } else {
        const unsigned px = div3((unsigned)cc);
        val = blend_lines(a, n, mask, line_s, (int)px, r0 + rr, cc - 3 * (int)px, val);
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
  const Band band = plan_band(a->W, a->dst_w, a->dst_h);
  p.pitch = band.pitch; p.R = band.R; p.nbands = band.nbands; p.xk_words = band.xk_words;
  PR_REQUIRE((long)a->N * p.nbands < (1l << 31), "pr_compose_video: batch too large (N = %d)", a->N);
  const size_t lds = ((size_t)p.R * p.pitch + p.xk_words + kMaxLines * kLineWords + 4) * 4;   // <= 48 KB (one row of W = 4096) + 8 KB + 400 B
  const int taps = band.taps;
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
