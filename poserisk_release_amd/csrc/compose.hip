// The canvas compositor behind both video entries (ABI 15 / 16), one launch a batch:
//   pr_compose_video   every canvas of <TITLE>_video -- the source frame with the track's box, area-resampled to dst_w x dst_h,
//                      beside a text panel.  Contract: section r2 of include/poserisk_hip.h (box, integer-exact area resample,
//                      panel text); tests/video_ref.py restates it in numpy and tests/test_video_gpu.py compares every byte.
//   pr_compose_people  every canvas of <TITLE>_people -- up to 16 people's boxes, each in its own colour, a short tag at each box
//                      drawn over the resampled image, beside a panel that lists the people of that frame.  Contract: section r3,
//                      which refers to r2 for everything the two share; tests/video_people_ref.py, tests/test_people_gpu.py.
// pr_compose_video IS pr_compose_people with K = 1 box slot, no tag lines and one colour for every canvas (r3's reduction
// property), and that is how it runs: its entry fills the same parameter block, the one colour packed into the block itself
// instead of a table on the device, so that it still uploads and allocates nothing.
//
// One workgroup owns a band of R destination rows of one canvas.  By its bytes the kernel should be HBM-bound (3 H W in,
// 3 dst_h (dst_w + panel_w) out per canvas) and both directions move 16 bytes per lane; measured, it is bound by the latency
// of the horizontal pass under the occupancy LDS allows (11 % of the byte floor at 800x450).
//   phase A  vertical pass.  A thread owns 16 consecutive bytes of the source rows (a byte is one channel of one pixel, so
//            the 3-byte interleave needs no shuffling on this axis), loads them from each of the few source rows a destination
//            row overlaps, paints the boxes, and sums them with the row weights oy into V[r][3 x + c] (u32, <= 255 H) in LDS.
//            The box paint is a loop over slots, in index order, later over earlier: a bit mask built once per workgroup from
//            the box table in LDS names the slots whose outline rows meet the band's source rows, and every 16-byte piece
//            narrows it, once for all its source rows, to the slots with an edge at its six pixels.
//   phase B  horizontal pass.  The band of the canvas is one contiguous byte range of `out`; a thread owns 16-byte-aligned
//            pieces of it.  A piece inside the image region that no tag of this band reaches: branch-free, the tap count a
//            template argument, 16 x T reads of V issued together, sum of ox V, the rounded division, one 16-byte store.  A panel
//            piece no line of this band reaches: zeros.  Pieces with text (on the image the tag lines blend over the resampled
//            byte), across the image's edge, a row's end or the band's ragged ends: byte by byte (the bytes of a piece that
//            belong to a neighbouring band are that band's).  Tags never reach the panel, panel lines never the image.
// The only LDS traffic of weight is V: phase A writes 16 consecutive dwords per lane (four ds_write_b128 at a lane stride of 64
// bytes), phase B gathers 2 - 4 taps per output byte at a lane stride of about 18 dwords; both shapes conflict across banks.
//
// The kernel's time follows its instruction schedule more closely than its source suggests.  While there were two kernels,
// moving the line table's entry, the box paint and the branch-free 16-byte image piece out of them into shared functions
// changed the single-box kernel's schedule and cost it 3.3 % at 64 x 800x450 (0.2575 against 0.2493 ms; the first two alone
// 0.8 %).  Those three pieces are therefore written out where they run, in the kernel's own body; the
// helpers below are force-inlined.  Time a change here at both of scripts/bench_video.py's shapes before keeping it.
#include "common.h"

// the workgroup's dynamic LDS block: V, the first-tap table, the line table, the box table (at file scope so that a host build
// can supply it)
extern __shared__ __attribute__((aligned(16))) unsigned pr_compose_lds[];

namespace pr {
namespace {

constexpr int kThreads = 256;
constexpr int kMaxRows = 8;               // destination rows per band at most
// Bytes of LDS for V: R = kVBudget / (4 * pitch), 1 <= R <= kMaxRows.  Measured at 64 x 800x450 (scripts/bench_video.py): 64 KB
// (R = 6, 2 workgroups a CU) 0.54 ms, 48 KB (R = 5, 3 a CU) 0.37 ms, 32 KB (R = 3, 5 a CU) 0.25 ms, 20 KB (R = 2, 7 a CU) 0.27 ms:
// the kernel lives on the waves in flight, until the bands get so thin that their shared source rows are read too often.
constexpr int kVBudget = 32 * 1024;
constexpr int kFar = 1 << 22;               // farther than any box edge or line origin that can touch a canvas
constexpr int kLineWords = 6;              // x0, canvas row of atlas row 0, size class, length, colour, advance
constexpr int kBoxWords = 5;               // x_min, y_min, x_max, y_max (clamped), colour
// the tables are sized for pr_compose_people's limits; pr_compose_video's entry holds L to PR_VIDEO_MAX_LINES
constexpr int kMaxLines = PR_PEOPLE_MAX_LINES;
constexpr int kMaxBoxes = PR_PEOPLE_MAX_BOXES;
constexpr int kTableWords = kMaxLines * kLineWords + kMaxBoxes * kBoxWords + 4;      // + tag, panel, box and box-edge masks
static_assert(kMaxLines <= 32 && kMaxBoxes <= 32, "the masks are one dword each");
static_assert(PR_VIDEO_MAX_LINES <= kMaxLines, "pr_compose_video's lines fit the line table");

struct Params {
  pr_compose_people_args a;
  int R, nbands, pitch;   // pitch: dwords per V row (3 W rounded up to 16)
  int xk_words;           // dwords of the first-tap table (dst_w u16, rounded up to 16 bytes)
  unsigned box_rgb;       // every slot's colour where a.box_rgb is null (pr_compose_video): channel c in bits 8 c .. 8 c + 7
};

__device__ __forceinline__ unsigned div3(unsigned v) { return (v * 43691u) >> 17; }   // exact below 65536

__device__ __forceinline__ int clamp_far(int v) { return min(max(v, -kFar), kFar); }

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

// 16 bytes of source row `src` (fewer than 16 valid at the row's end: the rest read as 0).
__device__ __forceinline__ void load_piece(uint8_t (&b)[16], const uint8_t* src, int nvalid) {
  if (nvalid == 16) {
    __builtin_memcpy(b, src, 16);                            // one 16-byte load (rows need not be 16-byte aligned)
  } else {
#pragma unroll
    for (int q = 0; q < 16; ++q) b[q] = q < nvalid ? src[q] : (uint8_t)0;
  }
}

// Whether one of the lines in `mask` reaches pixels xa .. xb of a row of the band.
__device__ __forceinline__ bool lines_reach(unsigned mask, const int (*line_s)[kLineWords], int xa, int xb) {
  bool hit = false;
  for (unsigned m = mask; m; m &= m - 1u) {
    const int* ln = line_s[__builtin_ctz(m)];
    hit = hit || (xb >= ln[0] && xa < ln[0] + ln[3] * ln[5]);
  }
  return hit;
}

// The lines in `mask`, in index order, over channel c of canvas pixel (x, y) whose value so far is val.
__device__ __forceinline__ unsigned blend_lines(const pr_compose_people_args& a, int n, unsigned mask, const int (*line_s)[kLineWords],
                                                int x, int y, int c, unsigned val) {
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
  return val;
}

// Byte cc of the image region of a destination row whose column sums are vrow, any tap count.
__device__ __forceinline__ unsigned image_byte(const pr_compose_people_args& a, const unsigned* vrow, const unsigned short* xk, int cc,
                                               unsigned D, float invD) {
  const unsigned i = div3((unsigned)cc);
  const int c = cc - 3 * (int)i;
  const int lo = (int)i * a.W, hi = lo + a.W;
  const unsigned* vr = vrow + c;
  int k = xk[i];
  unsigned S = 0u;
  for (int s0 = k * a.dst_w; s0 < hi; s0 += a.dst_w, ++k)
    S += (unsigned)(min(s0 + a.dst_w, hi) - max(s0, lo)) * vr[3 * k];
  return round_div(S, D, invD);
}

// T: the most source columns a destination column overlaps (its taps), 1 .. 4, or 0 for more: then every image byte takes the
// byte-by-byte path.
template <int T>
__global__ void __launch_bounds__(kThreads) compose_kernel(Params p) {
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
    // Entry tid of the canvas's line table; live: whether the line draws anything in canvas rows [r0, r0 + rows).  Origins are
    // any int32: beyond +-kFar a line cannot reach a canvas of <= 8192 x 4096 pixels with cells of <= 256 rows and <= 4096 * 256
    // columns, so clamping changes nothing and keeps the differences inside int32.
    const int* ln = a.lines + ((long)n * a.L + tid) * PR_VIDEO_LINE_INTS;
    const int cls = ln[2], len = min(ln[3], a.C);
    int adv = 1, ascent = 0;
#pragma unroll
    for (int s = 0; s < PR_VIDEO_MAX_CLASSES; ++s)
      if (cls == s) { adv = a.adv[s]; ascent = a.ascent[s]; }
    const int x0 = clamp_far(ln[0]), top = clamp_far(ln[1]) - ascent;
    int* ls = line_s[tid];
    ls[0] = x0; ls[1] = top; ls[2] = cls;
    ls[3] = len; ls[4] = ln[4]; ls[5] = adv;
    if ((unsigned)cls < (unsigned)a.S && len > 0 && top < r0 + rows && top + a.CH > r0)
      atomicOr(&masks[tid < a.L_img ? 0 : 1], 1u << tid);
  }
  // the source rows this band's destination rows overlap: jlo .. jhi
  const int jlo = (r0 * a.H) / a.dst_h, jhi = ((r0 + rows) * a.H - 1) / a.dst_h;
  if (a.box && tid >= 64 && tid < 64 + a.K) {
    const int k = tid - 64;
    const int* b = a.box + ((long)n * a.K + k) * 4;
    const bool has_box = b[2] >= b[0];
    // corners are any int32: clamped (after the x_max < x_min test) to where they are off every frame anyway, so that the +-1
    // and +-2 of the outline rule stay inside int32
    const int bx0 = clamp_far(b[0]), by0 = clamp_far(b[1]), bx1 = clamp_far(b[2]), by1 = clamp_far(b[3]);
    box_s[k][0] = bx0; box_s[k][1] = by0; box_s[k][2] = bx1; box_s[k][3] = by1;
    unsigned rgb = p.box_rgb;
    if (a.box_rgb) {
      const uint8_t* c = a.box_rgb + ((long)n * a.K + k) * 4;
      rgb = (unsigned)c[0] | (unsigned)c[1] << 8 | (unsigned)c[2] << 16;
    }
    box_s[k][4] = (int)rgb;
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
          // the outline of one box over the 16 bytes of source row j that start at pixel px0, channel ch0 (they span pixels
          // px0 .. px0 + 5: the per-byte test is skipped where the row or the span cannot touch the box)
          const int* bs = box_s[__builtin_ctz(m)];
          const int bx0 = bs[0], by0 = bs[1], bx1 = bs[2], by1 = bs[3];
          const unsigned rgb = (unsigned)bs[4];
          const bool row_outer = j >= by0 - 1 && j <= by1 + 1;
          const bool row_inner = j >= by0 + 2 && j <= by1 - 2;
          if (row_outer && (int)px0 <= bx1 + 1 && (int)px0 + 5 >= bx0 - 1) {
            int x = (int)px0, c = ch0;
#pragma unroll
            for (int q = 0; q < 16; ++q) {
              if (on_box(x, row_outer, row_inner, bx0, bx1)) b[q] = (uint8_t)(rgb >> (8 * c));
              if (++c == 3) { c = 0; ++x; }
            }
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
      // 16 bytes of the image region: every byte on its own and branch-free, so that the 16 table reads and the 16 T taps
      // issue together
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

// Both entries from here: the argument checks in `who`'s name, the band plan and the launch.  max_lines: the entry's limit on L;
// one_rgb: pr_compose_video's one colour (it has no colour table), else null.
int compose(const char* who, const pr_compose_people_args& a, int max_lines, const uint8_t* one_rgb, void* stream) {
  PR_REQUIRE(a.N >= 0, "%s: N = %d", who, a.N);
  if (a.N == 0) return PR_OK;
  PR_REQUIRE(a.out, "%s: null out", who);
  PR_REQUIRE(a.frames, "%s: null frames", who);
  PR_REQUIRE(a.n_frames >= 1, "%s: n_frames = %d", who, a.n_frames);
  PR_REQUIRE(a.H >= 1 && a.W >= 1 && a.H <= 4096 && a.W <= 4096, "%s: frame H x W = %d x %d outside 1..4096", who, a.H, a.W);
  PR_REQUIRE(a.dst_w >= 1 && a.dst_w <= 4096, "%s: dst_w = %d outside 1..4096", who, a.dst_w);
  PR_REQUIRE(a.dst_h >= 1 && a.dst_h <= 4096, "%s: dst_h = %d outside 1..4096", who, a.dst_h);
  PR_REQUIRE(a.panel_w >= 0 && a.panel_w <= 4096, "%s: panel_w = %d outside 0..4096", who, a.panel_w);
  PR_REQUIRE(a.K >= 1 && a.K <= kMaxBoxes, "%s: K = %d box slots outside 1..%d", who, a.K, kMaxBoxes);
  PR_REQUIRE(!a.box || a.box_rgb || one_rgb, "%s: box without box_rgb", who);
  PR_REQUIRE(a.L >= 0 && a.L <= max_lines, "%s: L = %d lines outside 0..%d", who, a.L, max_lines);
  PR_REQUIRE(a.L_img >= 0 && a.L_img <= a.L, "%s: L_img = %d tag lines outside 0..L = %d", who, a.L_img, a.L);
  if (a.L > 0) {
    PR_REQUIRE(a.lines && a.text && a.atlas, "%s: null lines, text or atlas with L = %d", who, a.L);
    PR_REQUIRE(a.C >= 1 && a.C <= 4096, "%s: C = %d codes per line outside 1..4096", who, a.C);
    PR_REQUIRE(a.S >= 1 && a.S <= PR_VIDEO_MAX_CLASSES, "%s: S = %d size classes outside 1..%d", who, a.S, PR_VIDEO_MAX_CLASSES);
    PR_REQUIRE(a.CH >= 1 && a.CW >= 1 && a.CH <= 256 && a.CW <= 256, "%s: atlas cell CH x CW = %d x %d outside 1..256", who, a.CH, a.CW);
    for (int s = 0; s < a.S; ++s) {
      PR_REQUIRE(a.adv[s] >= 1 && a.adv[s] <= a.CW, "%s: adv[%d] = %d outside 1..CW = %d", who, s, a.adv[s], a.CW);
      PR_REQUIRE(a.ascent[s] >= -4096 && a.ascent[s] <= 4096, "%s: ascent[%d] = %d", who, s, a.ascent[s]);
    }
  }
  PR_REQUIRE(a.src_idx || a.N <= a.n_frames, "%s: %d canvases for %d frames without src_idx", who, a.N, a.n_frames);
  // how a canvas is cut into bands, and the LDS tables' sizes
  Params p;
  p.a = a;
  p.box_rgb = one_rgb ? (unsigned)one_rgb[0] | (unsigned)one_rgb[1] << 8 | (unsigned)one_rgb[2] << 16 : 0u;
  p.pitch = (3 * a.W + 15) & ~15;
  p.R = std::min({kMaxRows, std::max(1, kVBudget / (4 * p.pitch)), a.dst_h});
  p.nbands = (a.dst_h + p.R - 1) / p.R;
  p.xk_words = ((a.dst_w * 2 + 15) & ~15) / 4;
  int taps = 0;                                 // the most source columns a destination column overlaps
  for (long i = 0; i < a.dst_w; ++i) taps = std::max(taps, (int)(((i + 1) * a.W + a.dst_w - 1) / a.dst_w - i * a.W / a.dst_w));
  PR_REQUIRE((long)a.N * p.nbands < (1l << 31), "%s: batch too large (N = %d)", who, a.N);
  const size_t lds = ((size_t)p.R * p.pitch + p.xk_words + kTableWords) * 4;   // <= 48 KB (one row of W = 4096) + 8 KB + 1.1 KB
  const dim3 grid((unsigned)((long)a.N * p.nbands)), block(kThreads);
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

}  // namespace
}  // namespace pr

extern "C" int pr_compose_video(const pr_compose_args* v, void* stream) {
  PR_REQUIRE(v, "pr_compose_video: null argument struct");
  // one box slot whose colour is v->box_rgb on every canvas (int32[N,4] is [N,1,4]), every line a panel line
  pr_compose_people_args a = {v->frames, v->src_idx, v->box, nullptr, v->lines, v->text, v->atlas, v->out, v->status,
                              v->N, v->n_frames, v->H, v->W, v->dst_h, v->dst_w, v->panel_w, 1, v->L, 0, v->C, v->S, v->CH, v->CW};
  std::copy(v->adv, v->adv + PR_VIDEO_MAX_CLASSES, a.adv);
  std::copy(v->ascent, v->ascent + PR_VIDEO_MAX_CLASSES, a.ascent);
  return pr::compose("pr_compose_video", a, PR_VIDEO_MAX_LINES, v->box_rgb, stream);
}

extern "C" int pr_compose_people(const pr_compose_people_args* a, void* stream) {
  PR_REQUIRE(a, "pr_compose_people: null argument struct");
  return pr::compose("pr_compose_people", *a, PR_PEOPLE_MAX_LINES, nullptr, stream);
}
