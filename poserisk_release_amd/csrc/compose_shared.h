// What the two canvas compositors share (csrc/compose.hip: pr_compose_video, one box; csrc/compose_people.hip:
// pr_compose_people, up to 16 boxes and tags on the image): the band plan, the rounded division, the outline rule, the overlap
// tables of the area resample and the coverage blend of a text line.  The contract is written once, above pr_compose_video in
// include/poserisk_hip.h.  `Args` is pr_compose_args or pr_compose_people_args, which name their common fields alike.  Include
// after common.h.
//
// The functions are force-inlined into the kernel that uses them.  Three pieces on the hot paths are MACROS instead -- the line
// table's entry, the box paint and the branch-free 16-byte image piece: as functions they changed compose_kernel's schedule and
// cost pr_compose_video 3.3 % at 64 x 800x450 (0.2575 against 0.2493 ms; the first two alone 0.8 %),
// while a macro leaves each kernel the tokens it would have written itself.
#pragma once

namespace pr {
namespace compose {

constexpr int kThreads = 256;
constexpr int kMaxRows = 8;               // destination rows per band at most
// Bytes of LDS for V: R = kVBudget / (4 * pitch), 1 <= R <= kMaxRows.  Measured at 64 x 800x450 (scripts/bench_video.py): 64 KB
// (R = 6, 2 workgroups a CU) 0.54 ms, 48 KB (R = 5, 3 a CU) 0.37 ms, 32 KB (R = 3, 5 a CU) 0.25 ms, 20 KB (R = 2, 7 a CU) 0.27 ms:
// the kernel lives on the waves in flight, until the bands get so thin that their shared source rows are read too often.
constexpr int kVBudget = 32 * 1024;
constexpr int kFar = 1 << 22;               // farther than any box edge or line origin that can touch a canvas
constexpr int kLineWords = 6;              // x0, canvas row of atlas row 0, size class, length, colour, advance

// How a canvas is cut into bands, and the LDS tables' sizes.
struct Band {
  int R, nbands, pitch;   // pitch: dwords per V row (3 W rounded up to 16)
  int xk_words;           // dwords of the first-tap table (dst_w u16, rounded up to 16 bytes)
  int taps;               // the most source columns a destination column overlaps
};

inline Band plan_band(int W, int dst_w, int dst_h) {
  Band b;
  b.pitch = (3 * W + 15) & ~15;
  b.R = std::min(kMaxRows, std::max(1, kVBudget / (4 * b.pitch)));
  b.R = std::min(b.R, dst_h);
  b.nbands = (dst_h + b.R - 1) / b.R;
  b.xk_words = ((dst_w * 2 + 15) & ~15) / 4;
  b.taps = 0;
  for (long i = 0; i < dst_w; ++i)
    b.taps = std::max(b.taps, (int)(((i + 1) * W + dst_w - 1) / dst_w - i * W / dst_w));
  return b;
}

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

// The outline of one box over the 16 bytes b of source row j that start at pixel px0, channel ch0 (they span pixels
// px0 .. px0 + 5: the per-byte test is skipped where the row or the span cannot touch the box).  rgb: channel c in bits 8 c ..
#define PR_COMPOSE_PAINT_BOX(b, j, px0, ch0, has_box, bx0, by0, bx1, by1, rgb)                                         \
  {                                                                                                                    \
    const bool row_outer = (has_box) && (j) >= (by0) - 1 && (j) <= (by1) + 1;                                          \
    const bool row_inner = (j) >= (by0) + 2 && (j) <= (by1) - 2;                                                       \
    if (row_outer && (int)(px0) <= (bx1) + 1 && (int)(px0) + 5 >= (bx0) - 1) {                                         \
      int x = (int)(px0), c = (ch0);                                                                                   \
      _Pragma("unroll") for (int q = 0; q < 16; ++q) {                                                                 \
        if (pr::compose::on_box(x, row_outer, row_inner, (bx0), (bx1))) (b)[q] = (uint8_t)((rgb) >> (8 * c));          \
        if (++c == 3) { c = 0; ++x; }                                                                                  \
      }                                                                                                                \
    }                                                                                                                  \
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

// Entry l of canvas n's line table into ls[kLineWords]; live (a bool of the caller's): whether the line draws anything in canvas
// rows [r0, r0 + rows).  Origins are any int32: beyond +-kFar a line cannot reach a canvas of <= 8192 x 4096 pixels with cells
// of <= 256 rows and <= 4096 * 256 columns, so clamping changes nothing and keeps the differences inside int32.
#define PR_COMPOSE_LOAD_LINE(a, n, l, ls, r0, rows, live)                                                              \
  {                                                                                                                    \
    const int* ln = (a).lines + ((long)(n) * (a).L + (l)) * PR_VIDEO_LINE_INTS;                                        \
    const int cls = ln[2], len = min(ln[3], (a).C);                                                                    \
    live = (unsigned)cls < (unsigned)(a).S && len > 0;                                                                 \
    int adv = 1, ascent = 0;                                                                                           \
    _Pragma("unroll") for (int s = 0; s < PR_VIDEO_MAX_CLASSES; ++s)                                                   \
      if (cls == s) { adv = (a).adv[s]; ascent = (a).ascent[s]; }                                                      \
    const int x0 = min(max(ln[0], -pr::compose::kFar), pr::compose::kFar);                                             \
    const int top = min(max(ln[1], -pr::compose::kFar), pr::compose::kFar) - ascent;                                   \
    (ls)[0] = x0; (ls)[1] = top; (ls)[2] = cls;                                                                        \
    (ls)[3] = len;   (ls)[4] = ln[4]; (ls)[5] = adv;                                                                   \
    live = live && top < (r0) + (rows) && top + (a).CH > (r0);                                                         \
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
template <class Args>
__device__ __forceinline__ unsigned blend_lines(const Args& a, int n, unsigned mask, const int (*line_s)[kLineWords], int x, int y,
                                                int c, unsigned val) {
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

// 16 bytes of the image region that start at byte `col` of a destination row whose column sums are vrow, stored to the
// 16-byte-aligned P: every byte on its own and branch-free, so that the 16 table reads and the 16 T taps issue together.
// T >= 1: the tap count.
#define PR_COMPOSE_IMAGE_PIECE(T, a, vrow, xk, col, D, invD, P)                                                        \
  {                                                                                                                    \
    unsigned w[4] = {0u, 0u, 0u, 0u};                                                                                  \
    _Pragma("unroll") for (int q = 0; q < 16; ++q) {                                                                   \
      const unsigned i = pr::compose::div3((unsigned)((col) + q));                                                     \
      const int c = (col) + q - 3 * (int)i;                                                                            \
      const int lo = (int)i * (a).W, hi = lo + (a).W;          /* this destination column in units of 1 / (W dst_w) */ \
      const int k0 = (xk)[i];                                                                                          \
      unsigned S = 0u;                                         /* <= 255 H W < 2^32 for H, W <= 4096: u32 is exact */  \
      _Pragma("unroll") for (int t = 0; t < (T); ++t) {                                                                \
        const int s0 = (k0 + t) * (a).dst_w;                   /* a tap past the column's last has weight 0 */         \
        const int wt = max(min(s0 + (a).dst_w, hi) - max(s0, lo), 0);                                                  \
        S += (unsigned)wt * (vrow)[3 * min(k0 + t, (a).W - 1) + c];                                                    \
      }                                                                                                                \
      w[q >> 2] |= pr::compose::round_div(S, (D), (invD)) << (8 * (q & 3));                                            \
    }                                                                                                                  \
    *(uint4*)__builtin_assume_aligned((P), 16) = make_uint4(w[0], w[1], w[2], w[3]);                                   \
  }

// Byte cc of the image region of a destination row whose column sums are vrow, any tap count.
template <class Args>
__device__ __forceinline__ unsigned image_byte(const Args& a, const unsigned* vrow, const unsigned short* xk, int cc, unsigned D,
                                               float invD) {
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

}  // namespace compose
}  // namespace pr
