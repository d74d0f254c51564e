// People video: every canvas of <TITLE>_people -- the source frame with up to 16 people's boxes, each in its own colour,
// area-resampled to dst_w x dst_h with a short tag at each box, beside a panel that lists the people of that frame -- composed
// in one launch.  The contract is section r3 of include/poserisk_hip.h (pr_compose_people), which refers to r2
// (pr_compose_video) for everything the two share; tests/video_people_ref.py restates it in numpy and
// tests/test_people_gpu.py compares every byte.
//
// The kernel is csrc/compose.hip's (read its head for the two phases and their LDS traffic) with two differences:
//   phase A  the box paint is a loop over slots, in index order, later over earlier: a bit mask built once per workgroup from the
//            box table in LDS names the slots whose outline rows meet the band's source rows, and every 16-byte piece narrows
//            it, once for all its source rows, to the slots with an edge at its six pixels.
//   phase B  an image piece that a tag of this band reaches takes the byte-by-byte path, where the tag lines blend over the
//            resampled byte; every other image piece is compose.hip's branch-free 16-byte path.  Tags never reach the panel,
//            panel lines never the image.
// What both kernels compute the same way is csrc/compose_shared.h.
#include "common.h"
#include "compose_shared.h"

// the workgroup's dynamic LDS block: V, the first-tap table, the line table, the box table (at file scope so that a host build
// can supply it)
extern __shared__ __attribute__((aligned(16))) unsigned pr_compose_lds[];

namespace pr {
namespace {

using namespace compose;
constexpr int kMaxLines = PR_PEOPLE_MAX_LINES;
constexpr int kMaxBoxes = PR_PEOPLE_MAX_BOXES;
constexpr int kBoxWords = 5;               // x_min, y_min, x_max, y_max (clamped), colour
constexpr int kTableWords = kMaxLines * kLineWords + kMaxBoxes * kBoxWords + 4;      // + tag, panel, box and box-edge masks
static_assert(kMaxLines <= 32 && kMaxBoxes <= 32, "the masks are one dword each");

struct PeopleParams {
  pr_compose_people_args a;
  int R, nbands, pitch;   // compose::Band's
  int xk_words;
};

// T: as compose_kernel's.
template <int T>
__global__ void __launch_bounds__(kThreads) compose_people_kernel(PeopleParams p) {
  unsigned* lds = pr_compose_lds;
  const pr_compose_people_args& a = p.a;
  unsigned* V = lds;                                               // [R][pitch]
  unsigned short* xk = (unsigned short*)(lds + p.R * p.pitch);     // [dst_w] first source column of destination column i
  unsigned* tables = lds + p.R * p.pitch + p.xk_words;
  int (*line_s)[kLineWords] = (int (*)[kLineWords])tables;                                   // [kMaxLines] lines of this canvas
  int (*box_s)[kBoxWords] = (int (*)[kBoxWords])(tables + kMaxLines * kLineWords);           // [kMaxBoxes] boxes of this canvas
  // masks: the tags, the panel lines, the boxes that reach this band, and those of them with a horizontal edge in it
  unsigned* masks = tables + kMaxLines * kLineWords + kMaxBoxes * kBoxWords;

  const int n = blockIdx.x / p.nbands, band = blockIdx.x - n * p.nbands;
  const int r0 = band * p.R, rows = min(p.R, a.dst_h - r0);
  const int tid = threadIdx.x;
  const int W3 = 3 * a.W;
  const int fi = a.src_idx ? a.src_idx[n] : n;
  const bool have = (unsigned)fi < (unsigned)a.n_frames;
  if (band == 0 && tid == 0 && a.status) a.status[n] = have ? 0 : 1;

  // ---- tables: first tap per destination column, the lines and the boxes that reach this band ----------------------------
  for (int i = tid; i < a.dst_w; i += kThreads) xk[i] = (unsigned short)((unsigned)(i * a.W) / (unsigned)a.dst_w);
  if (tid < 4) masks[tid] = 0u;
  __syncthreads();
  if (tid < a.L) {
    bool live;
    PR_COMPOSE_LOAD_LINE(a, n, tid, line_s[tid], r0, rows, live)
    if (live) atomicOr(&masks[tid < a.L_img ? 0 : 1], 1u << tid);
  }
  // the source rows this band's destination rows overlap: jlo .. jhi
  const int jlo = (r0 * a.H) / a.dst_h, jhi = ((r0 + rows) * a.H - 1) / a.dst_h;
  if (a.box && tid >= 64 && tid < 64 + a.K) {
    const int k = tid - 64;
    const int* b = a.box + ((long)n * a.K + k) * 4;
    const uint8_t* rgb = a.box_rgb + ((long)n * a.K + k) * 4;
    const bool has_box = b[2] >= b[0];
    // corners are any int32: clamped (after the x_max < x_min test) to where they are off every frame anyway, so that the +-1
    // and +-2 of the outline rule stay inside int32
    const int bx0 = clamp_far(b[0]), by0 = clamp_far(b[1]), bx1 = clamp_far(b[2]), by1 = clamp_far(b[3]);
    box_s[k][0] = bx0; box_s[k][1] = by0; box_s[k][2] = bx1; box_s[k][3] = by1;
    box_s[k][4] = (int)((unsigned)rgb[0] | (unsigned)rgb[1] << 8 | (unsigned)rgb[2] << 16);
    if (has_box && by1 + 1 >= jlo && by0 - 1 <= jhi) {
      atomicOr(&masks[2], 1u << k);
      // ... and whether one of its two horizontal edges (three rows each) does: where neither does, the band lies between
      // them and only the pieces at the vertical edges can be painted
      if ((by0 + 1 >= jlo && by0 - 1 <= jhi) || (by1 + 1 >= jlo && by1 - 1 <= jhi)) atomicOr(&masks[3], 1u << k);
    }
  }
  __syncthreads();

  // ---- phase A: V[r][xc] = sum_j oy[r][j] boxed_src[j][xc] ---------------------------------------------------------------
  const int npieces = p.pitch >> 4;
  const unsigned box_mask = masks[2], edge_mask = masks[3];
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
      // the slots that can paint one of this piece's pixels px0 .. px0 + 5 in some row of the band: those whose columns
      // [x_min - 1, x_max + 1] meet them and that have a horizontal edge in the band or a vertical edge (three columns) here
      unsigned mine = 0u;
      for (unsigned m = box_mask; m; m &= m - 1u) {
        const int k = __builtin_ctz(m);
        const int bx0 = box_s[k][0], bx1 = box_s[k][2], xa = (int)px0, xb = (int)px0 + 5;
        const bool at_edge = (xa <= bx0 + 1 && xb >= bx0 - 1) || (xa <= bx1 + 1 && xb >= bx1 - 1);
        if (xa <= bx1 + 1 && xb >= bx0 - 1 && (((edge_mask >> k) & 1u) || at_edge)) mine |= 1u << k;
      }
      for (int j = lo / a.dst_h; j * a.dst_h < hi; ++j) {
        const unsigned oy = (unsigned)(min((j + 1) * a.dst_h, hi) - max(j * a.dst_h, lo));
        const uint8_t* src = frame + (long)j * W3 + xc0;
        uint8_t b[16];
        load_piece(b, src, nvalid);
        for (unsigned m = mine; m; m &= m - 1u) {                  // in index order: later over earlier
          const int* bs = box_s[__builtin_ctz(m)];
          PR_COMPOSE_PAINT_BOX(b, j, px0, ch0, true, bs[0], bs[1], bs[2], bs[3], (unsigned)bs[4])
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
  const unsigned tag_mask = masks[0], panel_mask = masks[1];
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
    const int xa = (int)div3((unsigned)col), xb = (int)div3((unsigned)(col + 15));   // the piece's pixels, when whole
    if (T > 0 && whole && col + 16 <= img_bytes && !lines_reach(tag_mask, line_s, xa, xb)) {
      const unsigned* vrow = V + r * p.pitch;
      PR_COMPOSE_IMAGE_PIECE((T > 0 ? T : 1), a, vrow, xk, col, D, invD, P)
      continue;
    }
    if (whole && col >= img_bytes && !lines_reach(panel_mask, line_s, xa, xb)) {
      *(uint4*)__builtin_assume_aligned(P, 16) = make_uint4(0u, 0u, 0u, 0u);      // panel: black where no line of this band is
      continue;
    }
    // everything else -- pieces with text, pieces across the image's edge, a row's end or the band's ends -- byte by byte
    int rr = r, cc = col;
#pragma unroll 1
    for (int q = first - off0; q < 16 && off0 + q < nbytes; ++q) {
      const unsigned px = div3((unsigned)cc);
      const int c = cc - 3 * (int)px;
      unsigned val;
      if (cc < img_bytes) {
        val = image_byte(a, V + rr * p.pitch, xk, cc, D, invD);
        val = blend_lines(a, n, tag_mask, line_s, (int)px, r0 + rr, c, val);
      } else {
        val = blend_lines(a, n, panel_mask, line_s, (int)px, r0 + rr, c, 0u);
      }
      P[q] = (uint8_t)val;
      if (++cc == rowbytes) { cc = 0; ++rr; }
    }
  }
}

}  // namespace
}  // namespace pr

extern "C" int pr_compose_people(const pr_compose_people_args* a, void* stream) {
  using namespace pr;
  PR_REQUIRE(a, "pr_compose_people: null argument struct");
  PR_REQUIRE(a->N >= 0, "pr_compose_people: N = %d", a->N);
  if (a->N == 0) return PR_OK;
  PR_REQUIRE(a->out, "pr_compose_people: null out");
  PR_REQUIRE(a->frames, "pr_compose_people: null frames");
  PR_REQUIRE(a->n_frames >= 1, "pr_compose_people: n_frames = %d", a->n_frames);
  PR_REQUIRE(a->H >= 1 && a->W >= 1 && a->H <= 4096 && a->W <= 4096, "pr_compose_people: frame H x W = %d x %d outside 1..4096",
             a->H, a->W);
  PR_REQUIRE(a->dst_w >= 1 && a->dst_w <= 4096, "pr_compose_people: dst_w = %d outside 1..4096", a->dst_w);
  PR_REQUIRE(a->dst_h >= 1 && a->dst_h <= 4096, "pr_compose_people: dst_h = %d outside 1..4096", a->dst_h);
  PR_REQUIRE(a->panel_w >= 0 && a->panel_w <= 4096, "pr_compose_people: panel_w = %d outside 0..4096", a->panel_w);
  PR_REQUIRE(a->K >= 1 && a->K <= PR_PEOPLE_MAX_BOXES, "pr_compose_people: K = %d box slots outside 1..%d", a->K, PR_PEOPLE_MAX_BOXES);
  PR_REQUIRE(!a->box || a->box_rgb, "pr_compose_people: box without box_rgb");
  PR_REQUIRE(a->L >= 0 && a->L <= PR_PEOPLE_MAX_LINES, "pr_compose_people: L = %d lines outside 0..%d", a->L, PR_PEOPLE_MAX_LINES);
  PR_REQUIRE(a->L_img >= 0 && a->L_img <= a->L, "pr_compose_people: L_img = %d tag lines outside 0..L = %d", a->L_img, a->L);
  if (a->L > 0) {
    PR_REQUIRE(a->lines && a->text && a->atlas, "pr_compose_people: null lines, text or atlas with L = %d", a->L);
    PR_REQUIRE(a->C >= 1 && a->C <= 4096, "pr_compose_people: C = %d codes per line outside 1..4096", a->C);
    PR_REQUIRE(a->S >= 1 && a->S <= PR_VIDEO_MAX_CLASSES, "pr_compose_people: S = %d size classes outside 1..%d", a->S,
               PR_VIDEO_MAX_CLASSES);
    PR_REQUIRE(a->CH >= 1 && a->CW >= 1 && a->CH <= 256 && a->CW <= 256, "pr_compose_people: atlas cell CH x CW = %d x %d outside 1..256",
               a->CH, a->CW);
    for (int s = 0; s < a->S; ++s) {
      PR_REQUIRE(a->adv[s] >= 1 && a->adv[s] <= a->CW, "pr_compose_people: adv[%d] = %d outside 1..CW = %d", s, a->adv[s], a->CW);
      PR_REQUIRE(a->ascent[s] >= -4096 && a->ascent[s] <= 4096, "pr_compose_people: ascent[%d] = %d", s, a->ascent[s]);
    }
  }
  PR_REQUIRE(a->src_idx || a->N <= a->n_frames, "pr_compose_people: %d canvases for %d frames without src_idx", a->N, a->n_frames);
  PeopleParams p;
  p.a = *a;
  const Band band = plan_band(a->W, a->dst_w, a->dst_h);
  p.pitch = band.pitch; p.R = band.R; p.nbands = band.nbands; p.xk_words = band.xk_words;
  PR_REQUIRE((long)a->N * p.nbands < (1l << 31), "pr_compose_people: batch too large (N = %d)", a->N);
  const size_t lds = ((size_t)p.R * p.pitch + p.xk_words + kTableWords) * 4;   // <= 48 KB (one row of W = 4096) + 8 KB + 1.1 KB
  const dim3 grid((unsigned)((long)a->N * p.nbands)), block(kThreads);
  hipStream_t s = (hipStream_t)stream;
  switch (band.taps) {
    case 1: hipLaunchKernelGGL(compose_people_kernel<1>, grid, block, lds, s, p); break;
    case 2: hipLaunchKernelGGL(compose_people_kernel<2>, grid, block, lds, s, p); break;
    case 3: hipLaunchKernelGGL(compose_people_kernel<3>, grid, block, lds, s, p); break;
    case 4: hipLaunchKernelGGL(compose_people_kernel<4>, grid, block, lds, s, p); break;
    default: hipLaunchKernelGGL(compose_people_kernel<0>, grid, block, lds, s, p); break;
  }
  return check_launch("compose_people_kernel");
}
