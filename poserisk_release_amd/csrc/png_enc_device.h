// The PNG encoder's device half written ONCE (include/poserisk_hip.h, section j5): the filters, the adaptive choice, the token
// rule, the code construction, the bit layout, the stored fallback and the checksum algebra, templated on a wave policy P:
//   EncWave64 (csrc/png_enc.hip)  64 lanes, one wavefront a workgroup, cross-lane operations, the scratch in LDS;
//   EncLane1  (below)             one lane, plain C++: what tests/native/png_enc_native.cc compiles with g++ under ASan + UBSan.
// A policy supplies: L (lanes), lane(), sync() (the scratch writes of the wave's other lanes are visible), ballot(pred),
// scan_add(v) (inclusive prefix sum over the lanes), reduce_add(v), reduce_xor(v) (the total, in every lane), last(v) (the last
// lane's value), or_word(p, v) and add_word(p, v) (scratch words that several lanes may combine into: integer OR and integer
// sum, so the result does not depend on the order).  Loops over positions run `for (base = 0; base < n; base += L)` with the
// lane's position base + lane(), so that every lane reaches every cross-lane operation.
//
// What the one-lane form does not cover: the cross-lane operations themselves and the combining of words several lanes share.
// tests/test_png_encode_gpu.py (byte-exact cases, guard bands) covers those.
#pragma once
#include <cstdint>
#include <cstring>

#include "../../include/poserisk_hip.h"

// PR_PNG_ENC_HOST_ONLY: set by csrc/png_enc_host.cc, which the library's build hands to the HIP driver without the HIP runtime's header
#if defined(__HIPCC__) && !defined(PR_PNG_ENC_HOST_ONLY)
#define PR_PE_HD __host__ __device__ __forceinline__
#else
#define PR_PE_HD inline
#endif

namespace pr {
namespace pngenc {

constexpr int kSeg = PR_PNG_ENC_SEGMENT;
constexpr int kStage = kSeg + 16;        // a segment's staging area: at most 5 + kSeg bytes are written, whole dwords are read
constexpr int kOutWords = kStage / 4 + 2;
constexpr int kLitSyms = 286, kClSyms = 19;
constexpr uint32_t kPoly = 0xEDB88320u;
constexpr uint32_t kAdler = 65521u;

struct SegRec {   // what the segment kernel leaves for the assemble kernel
  uint32_t len;   // bytes in the staging area
  uint32_t crc;   // the CRC register after those bytes, started from 0 (no inversion)
  uint32_t a, b;  // Adler partial sums of the segment's n filtered bytes: sum x_i and sum (n - i) x_i, mod 65521
};

// ---- the workspace: one layout for the host half and the device half ---------------------------------------------------------
struct EncLayout {
  int nseg;
  int64_t raw;
  size_t stage, rec, seg_off, rowf, fstate, total;
  int rowf_stride;
};
inline bool enc_layout(int F, int H, int W, EncLayout* l) {
  if (F <= 0 || F > 65535 || H < 1 || W < 1 || H > PR_PNG_MAX_SIDE || W > PR_PNG_MAX_SIDE) return false;
  l->raw = (int64_t)H * (1 + 3 * (int64_t)W);
  l->nseg = (int)((l->raw + kSeg - 1) / kSeg);
  l->rowf_stride = (H + 15) & ~15;
  auto up = [](size_t n) { return (n + 15) & ~(size_t)15; };
  const size_t f = (size_t)F, ns = (size_t)l->nseg;
  size_t o = 0;
  l->stage = o, o += f * ns * kStage;
  l->rec = o, o += up(f * ns * sizeof(SegRec));
  l->seg_off = o, o += up(f * ns * 4);
  l->rowf = o, o += f * (size_t)l->rowf_stride;
  l->fstate = o, o += up(f * 4);
  l->total = o;
  return true;
}

// ---- CRC-32 algebra (reflected representation: bit 31 is x^0) -----------------------------------------------------------------
PR_PE_HD uint32_t multmodp(uint32_t a, uint32_t b) {   // a * b mod the polynomial
  uint32_t p = 0;
  for (int i = 0; i < 32; ++i) {
    if (a & (0x80000000u >> i)) p ^= b;
    b = (b & 1u) ? (b >> 1) ^ kPoly : b >> 1;
  }
  return p;
}
PR_PE_HD uint32_t xpow_bytes(const uint32_t* pow2k, uint64_t n) {   // x^(8 n), from pow2k[k] = x^(2^k)
  uint32_t p = 0x80000000u;
  for (int k = 3; n; n >>= 1, ++k)
    if (n & 1u) p = multmodp(pow2k[k & 31], p);
  return p;
}
PR_PE_HD uint32_t crc_byte(uint32_t c, uint32_t byte) {   // the register after one more byte, without a table
  c ^= byte;
  for (int k = 0; k < 8; ++k) c = (c & 1u) ? (c >> 1) ^ kPoly : c >> 1;
  return c;
}

// ---- filters -----------------------------------------------------------------------------------------------------------------
struct FilterSrc {        // the filtered stream of one frame, computed from the raw pixels where it is asked for
  const uint8_t* frame;   // u8[H,W,3]
  int H, W, bgr;
  int fixed;              // 0..4, or 5: take the row's filter from rowf
  const uint8_t* rowf;    // [H], adaptive only

  PR_PE_HD int raw(int row, int j) const {   // byte j of the row as RGB
    const int64_t at = (int64_t)row * 3 * W + j;
    return frame[bgr ? at + 2 - 2 * (j % 3) : at];
  }
  PR_PE_HD static int paeth(int a, int b, int c) {
    const int q = a + b - c;
    const int pa = q > a ? q - a : a - q, pb = q > b ? q - b : b - q, pc = q > c ? q - c : c - q;
    return (pa <= pb && pa <= pc) ? a : pb <= pc ? b : c;
  }
  PR_PE_HD int apply(int t, int row, int j) const {
    const int x = raw(row, j);
    if (t == 0) return x;
    const int a = j >= 3 ? raw(row, j - 3) : 0, b = row > 0 ? raw(row - 1, j) : 0;
    if (t == 1) return (x - a) & 255;
    if (t == 2) return (x - b) & 255;
    if (t == 3) return (x - ((a + b) >> 1)) & 255;
    const int c = (j >= 3 && row > 0) ? raw(row - 1, j - 3) : 0;
    return (x - paeth(a, b, c)) & 255;
  }
  PR_PE_HD int at(int64_t off) const {   // byte `off` of the filtered stream, off < H (1 + 3 W)
    const uint32_t stride = 1u + 3u * (uint32_t)W, o = (uint32_t)off;   // the stream is below 4096 * 12289 < 2^26 bytes: 32-bit division
    const int row = (int)(o / stride), col = (int)(o - (uint32_t)row * stride);
    const int t = fixed < 5 ? fixed : rowf[row];
    return col == 0 ? t : apply(t, row, col - 1);
  }
};

// The adaptive choice of one row (the same value in every lane).
template <class P>
PR_PE_HD int choose_row(const P& p, const FilterSrc& src, int row) {
  uint32_t s0 = 0, s1 = 0, s2 = 0, s3 = 0, s4 = 0;
  const int n = 3 * src.W;
  auto mag = [](int v) { return (uint32_t)(v < 128 ? v : 256 - v); };
  for (int j = p.lane(); j < n; j += P::L) {
    s0 += mag(src.apply(0, row, j));
    s1 += mag(src.apply(1, row, j));
    s2 += mag(src.apply(2, row, j));
    s3 += mag(src.apply(3, row, j));
    s4 += mag(src.apply(4, row, j));
  }
  s0 = p.reduce_add(s0), s1 = p.reduce_add(s1), s2 = p.reduce_add(s2), s3 = p.reduce_add(s3), s4 = p.reduce_add(s4);
  int best = 0;
  uint32_t m = s0;
  if (s1 < m) m = s1, best = 1;
  if (s2 < m) m = s2, best = 2;
  if (s3 < m) m = s3, best = 3;
  if (s4 < m) m = s4, best = 4;
  return best;
}

// ---- a segment's scratch: LDS on the device ----------------------------------------------------------------------------------
template <int L>
struct SegScratch {
  uint32_t out[kOutWords];             // the segment's bytes as they go to the staging area (bits LSB first = little-endian words)
  uint8_t in[kSeg];                    // its filtered bytes
  uint64_t mask[kSeg / L];             // bit k of word w: position w L + k starts a run
  uint16_t last_start[kSeg / L];       // the last run start in words <= w
  uint16_t next_start[kSeg / L + 1];   // the first run start in words >= w, or n
  uint32_t hist[288];
  uint16_t code[288];                  // bit-reversed
  uint8_t len[288];
  uint16_t sorted[288];
  uint32_t weight[2 * 288];
  uint16_t parent[2 * 288], depth[2 * 288];
  uint32_t count[16];
  uint8_t cl_sym[320], cl_extra[320];
  uint32_t cl_hist[kClSyms];
  uint16_t cl_code[kClSyms], cl_sorted[kClSyms];
  uint8_t cl_len[kClSyms];
  uint32_t crc_table[256];
  int32_t n_cl, dynamic, head_bits, out_len;
};

struct EncLane1 {
  static constexpr int L = 1;
  PR_PE_HD int lane() const { return 0; }
  PR_PE_HD void sync() const {}
  PR_PE_HD uint64_t ballot(bool b) const { return b ? 1u : 0u; }
  PR_PE_HD uint32_t scan_add(uint32_t v) const { return v; }
  PR_PE_HD uint32_t reduce_add(uint32_t v) const { return v; }
  PR_PE_HD uint32_t reduce_xor(uint32_t v) const { return v; }
  PR_PE_HD uint32_t last(uint32_t v) const { return v; }
  PR_PE_HD void or_word(uint32_t* p, uint32_t v) const { *p |= v; }
  PR_PE_HD void add_word(uint32_t* p, uint32_t v) const { *p += v; }
};

// ---- code construction (serial: one lane calls these) ------------------------------------------------------------------------
// Steps 2 - 4 of the construction: sorted[0..n) are the used symbols in (count, symbol) order.
PR_PE_HD void tree_lengths(const uint32_t* hist, const uint16_t* sorted, int n, int nsym, int limit, uint8_t* len, uint32_t* w,
                           uint16_t* parent, uint16_t* depth, uint32_t* count) {
  for (int s = 0; s < nsym; ++s) len[s] = 0;
  if (n == 0) return;
  if (n == 1) {
    len[sorted[0]] = 1;
    return;
  }
  for (int i = 0; i < n; ++i) w[i] = hist[sorted[i]];
  int leaf = 0, ih = n;
  for (int k = n; k < 2 * n - 1; ++k) {
    int pick[2];
    for (int j = 0; j < 2; ++j) pick[j] = (leaf < n && (ih >= k || w[leaf] < w[ih])) ? leaf++ : ih++;
    w[k] = w[pick[0]] + w[pick[1]];
    parent[pick[0]] = parent[pick[1]] = (uint16_t)k;
  }
  depth[2 * n - 2] = 0;
  for (int i = 2 * n - 3; i >= 0; --i) depth[i] = (uint16_t)(depth[parent[i]] + 1);
  for (int d = 0; d <= limit; ++d) count[d] = 0;
  for (int i = 0; i < n; ++i) ++count[depth[i] < limit ? depth[i] : limit];
  uint32_t total = 0;
  for (int d = 1; d <= limit; ++d) total += count[d] << (limit - d);
  for (; total > (1u << limit); --total) {
    --count[limit];
    for (int d = limit - 1; d >= 1; --d)
      if (count[d]) {
        --count[d];
        count[d + 1] += 2;
        break;
      }
  }
  int j = 0;
  for (int d = limit; d >= 1; --d)
    for (uint32_t c = 0; c < count[d]; ++c) len[sorted[j++]] = (uint8_t)d;
}

// Step 5: canonical codes, stored bit-reversed (deflate sends a code's most significant bit first).
PR_PE_HD void canonical_codes(const uint8_t* len, int nsym, int limit, uint16_t* code, uint32_t* count) {
  for (int d = 0; d <= limit; ++d) count[d] = 0;
  for (int s = 0; s < nsym; ++s) ++count[len[s]];
  count[0] = 0;
  uint32_t c = 0, prev = 0;
  for (int d = 1; d <= limit; ++d) {   // count[d] becomes the first code of length d
    c = (c + prev) << 1;
    prev = count[d];
    count[d] = c;
  }
  for (int s = 0; s < nsym; ++s) {
    const int n = len[s];
    if (!n) continue;
    uint32_t v = count[n]++, r = 0;
    for (int i = 0; i < n; ++i, v >>= 1) r = r << 1 | (v & 1u);
    code[s] = (uint16_t)r;
  }
}

// The used symbols in (count, symbol) order by their ranks: every lane ranks its own symbols against all.
template <class P>
PR_PE_HD void rank_sort(const P& p, const uint32_t* hist, int nsym, uint16_t* sorted) {
  for (int s = p.lane(); s < nsym; s += P::L) {
    const uint32_t c = hist[s];
    if (!c) continue;
    int rank = 0;
    for (int t = 0; t < nsym; ++t) {
      const uint32_t d = hist[t];
      rank += d && (d < c || (d == c && t < s));
    }
    sorted[rank] = (uint16_t)s;
  }
}

// length 3..258 -> its symbol, extra bits and their value
PR_PE_HD void length_symbol(int length, int* sym, int* ebits, uint32_t* extra) {
  const uint32_t v = (uint32_t)length - 3u;
  if (length == 258) {
    *sym = 285, *ebits = 0, *extra = 0;
  } else if (v < 8) {
    *sym = 257 + (int)v, *ebits = 0, *extra = 0;
  } else {
    const int eb = 31 - __builtin_clz(v) - 2;
    *sym = 257 + 4 * (eb + 1) + (int)((v >> eb) & 3u);
    *ebits = eb;
    *extra = v & ((1u << eb) - 1u);
  }
}
PR_PE_HD int symbol_extra_bits(int sym) { return (sym < 265 || sym == 285) ? 0 : (sym - 261) >> 2; }

struct Token {
  int kind;   // 0: inside a match, 1: literal, 2: match
  int sym, ebits;
  uint32_t extra;
};

// The token that starts at position i of the segment (section j5, Tokens); the segment's end is next_start's last entry.
template <int L>
PR_PE_HD Token token_at(const SegScratch<L>& s, int i) {
  Token t;
  t.kind = 1, t.sym = s.in[i], t.ebits = 0, t.extra = 0;
  const int w = i / L, bit = i % L;
  const uint64_t upto = (2ull << bit) - 1ull;   // bits 0..bit
  const uint64_t here = s.mask[w];
  int start;
  if (here & upto) start = w * L + 63 - __builtin_clzll(here & upto);
  else start = s.last_start[w - 1];             // word 0 holds position 0, which starts a run
  const int o = i - start;
  if (o == 0) return t;
  int end;
  if (here & ~upto) end = w * L + __builtin_ctzll(here & ~upto);
  else end = s.next_start[w + 1];
  const int r = o - 1, R = end - start - 1;
  const int blk = r / 258 * 258;
  const int blen = R - blk < 258 ? R - blk : 258;
  if (blen < 3) return t;
  if (r != blk) {
    t.kind = 0;
    return t;
  }
  t.kind = 2;
  length_symbol(blen, &t.sym, &t.ebits, &t.extra);
  return t;
}

PR_PE_HD void put_serial(uint32_t* out, int* pos, uint32_t v, int nbits) {   // one lane, nbits <= 24
  const int at = *pos, sh = at & 31;
  const uint64_t x = (uint64_t)v << sh;
  out[at >> 5] |= (uint32_t)x;
  if (x >> 32) out[(at >> 5) + 1] |= (uint32_t)(x >> 32);
  *pos = at + nbits;
}

// The code-length sequence of len[0..hlit) and the distance length 1 (section j5, Codes) -> s.cl_sym / s.cl_extra / s.n_cl
template <int L>
PR_PE_HD void length_sequence(SegScratch<L>& s, int hlit) {
  int k = 0, i = 0;
  const int total = hlit + 1;
  auto at = [&](int q) { return q < hlit ? (int)s.len[q] : 1; };
  while (i < total) {
    const int v = at(i);
    int j = i;
    while (j < total && at(j) == v) ++j;
    int run = j - i;
    if (v == 0) {
      while (run >= 3) {
        const int take = run >= 11 ? (run < 138 ? run : 138) : run;
        s.cl_sym[k] = run >= 11 ? 18 : 17;
        s.cl_extra[k++] = (uint8_t)(take - (run >= 11 ? 11 : 3));
        run -= take;
      }
    } else {
      s.cl_sym[k] = (uint8_t)v, s.cl_extra[k++] = 0;
      --run;
      while (run >= 3) {
        const int take = run < 6 ? run : 6;
        s.cl_sym[k] = 16, s.cl_extra[k++] = (uint8_t)(take - 3);
        run -= take;
      }
    }
    for (; run > 0; --run) s.cl_sym[k] = (uint8_t)v, s.cl_extra[k++] = 0;
    i = j;
  }
  s.n_cl = k;
}

// ---- one segment -------------------------------------------------------------------------------------------------------------
// Bytes [begin, begin + n) of src's filtered stream -> at most 5 + n bytes at `stage` (exactly rec->len of them) and *rec.
template <class P>
PR_PE_HD void encode_segment(const P& p, SegScratch<P::L>& s, const FilterSrc& src, int64_t begin, int n, bool last, int mode,
                             const uint32_t* crc_pow, uint8_t* stage, SegRec* rec) {
  constexpr int L = P::L;
  const int lane = p.lane();
  uint8_t* const ob = (uint8_t*)s.out;
  constexpr uint8_t kClOrder[kClSyms] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
  // 1. the filtered bytes, their Adler partial sums, cleared scratch, the CRC table
  uint32_t a = 0;
  uint64_t b64 = 0;   // (n - i) x over up to n positions: above 2^32 in the one-lane form
  for (int i = lane; i < n; i += L) {
    const uint32_t x = (uint32_t)src.at(begin + i);
    s.in[i] = (uint8_t)x;
    a += x;
    b64 += (uint64_t)(n - i) * x;
  }
  for (int i = lane; i < (n + 5 + 3) / 4 + 1; i += L) s.out[i] = 0;
  for (int i = lane; i < 288; i += L) s.hist[i] = 0;
  for (int i = lane; i < 256; i += L) {
    uint32_t c = (uint32_t)i;
    for (int k = 0; k < 8; ++k) c = (c & 1u) ? (c >> 1) ^ kPoly : c >> 1;
    s.crc_table[i] = c;
  }
  if (lane == 0) s.dynamic = 0;
  a = p.reduce_add(a % kAdler) % kAdler;
  const uint32_t b = p.reduce_add((uint32_t)(b64 % kAdler)) % kAdler;
  p.sync();
  if (mode == PR_PNG_ENC_RLE) {
    // 2. run starts as bit masks, and for every word the nearest start on either side
    const int nw = (n + L - 1) / L;
    for (int base = 0; base < n; base += L) {
      const int i = base + lane;
      const uint64_t m = p.ballot(i < n && (i == 0 || s.in[i] != s.in[i - 1]));
      if (lane == 0) s.mask[base / L] = m;
    }
    p.sync();
    if (lane == 0) {
      int at = 0;
      for (int w = 0; w < nw; ++w) {
        if (s.mask[w]) at = w * L + 63 - __builtin_clzll(s.mask[w]);
        s.last_start[w] = (uint16_t)at;
      }
      at = n;
      s.next_start[nw] = (uint16_t)at;
      for (int w = nw - 1; w >= 0; --w) {
        if (s.mask[w]) at = w * L + __builtin_ctzll(s.mask[w]);
        s.next_start[w] = (uint16_t)at;
      }
    }
    p.sync();
    // 3. the histogram
    for (int base = 0; base < n; base += L) {
      const int i = base + lane;
      if (i < n) {
        const Token t = token_at<L>(s, i);
        if (t.kind) p.add_word(&s.hist[t.sym], 1u);
      }
    }
    if (lane == 0) p.add_word(&s.hist[256], 1u);
    p.sync();
    // 4. code lengths and codes, the code-length code, the size of it all
    rank_sort(p, s.hist, kLitSyms, s.sorted);
    p.sync();
    if (lane == 0) {
      int used = 0, hlit = 257;
      for (int q = 0; q < kLitSyms; ++q)
        if (s.hist[q]) ++used, hlit = q + 1 > hlit ? q + 1 : hlit;
      tree_lengths(s.hist, s.sorted, used, kLitSyms, 15, s.len, s.weight, s.parent, s.depth, s.count);
      canonical_codes(s.len, kLitSyms, 15, s.code, s.count);
      length_sequence<L>(s, hlit);
      for (int q = 0; q < kClSyms; ++q) s.cl_hist[q] = 0;
      for (int q = 0; q < s.n_cl; ++q) ++s.cl_hist[s.cl_sym[q]];
      int cl_used = 0;
      for (int q = 0; q < kClSyms; ++q) cl_used += s.cl_hist[q] != 0;
      EncLane1 one;
      rank_sort(one, s.cl_hist, kClSyms, s.cl_sorted);
      tree_lengths(s.cl_hist, s.cl_sorted, cl_used, kClSyms, 7, s.cl_len, s.weight, s.parent, s.depth, s.count);
      canonical_codes(s.cl_len, kClSyms, 7, s.cl_code, s.count);
      int hclen = 4;
      for (int q = 4; q < kClSyms; ++q)
        if (s.cl_len[kClOrder[q]]) hclen = q + 1;
      uint32_t bits = 3 + 14 + 3 * (uint32_t)hclen;
      for (int q = 0; q < s.n_cl; ++q) {
        const int sym = s.cl_sym[q];
        bits += s.cl_len[sym] + (sym == 16 ? 2 : sym == 17 ? 3 : sym == 18 ? 7 : 0);
      }
      for (int q = 0; q < kLitSyms; ++q) bits += s.hist[q] * (s.len[q] + symbol_extra_bits(q) + (q > 256 ? 1 : 0));
      const uint32_t bytes = last ? (bits + 7) / 8 : (bits + 3 + 7) / 8 + 4;
      s.dynamic = bytes < 5u + (uint32_t)n;
      if (s.dynamic) {
        int pos = 0;
        put_serial(s.out, &pos, (last ? 1u : 0u) | 2u << 1, 3);
        put_serial(s.out, &pos, (uint32_t)(hlit - 257), 5);
        put_serial(s.out, &pos, 0u, 5);
        put_serial(s.out, &pos, (uint32_t)(hclen - 4), 4);
        for (int q = 0; q < hclen; ++q) put_serial(s.out, &pos, s.cl_len[kClOrder[q]], 3);
        for (int q = 0; q < s.n_cl; ++q) {
          const int sym = s.cl_sym[q];
          put_serial(s.out, &pos, s.cl_code[sym], s.cl_len[sym]);
          if (sym >= 16) put_serial(s.out, &pos, s.cl_extra[q], sym == 16 ? 2 : sym == 17 ? 3 : 7);
        }
        s.head_bits = pos;
      }
    }
    p.sync();
  }
  if (s.dynamic) {
    // 5. every token at its bit offset: a prefix sum of the bit counts, 64 positions a step
    uint32_t base_bits = (uint32_t)s.head_bits;
    for (int base = 0; base < n; base += L) {
      const int i = base + lane;
      Token t;
      t.kind = 0;
      if (i < n) t = token_at<L>(s, i);
      uint64_t v = 0;
      uint32_t nb = 0;
      if (t.kind) {
        const uint32_t cl = s.len[t.sym];
        v = (uint64_t)s.code[t.sym] | (uint64_t)t.extra << cl;   // a match: the distance code 0 follows as one 0 bit
        nb = cl + (uint32_t)t.ebits + (t.kind == 2 ? 1u : 0u);
      }
      const uint32_t incl = p.scan_add(nb);
      if (nb) {
        const uint32_t at = base_bits + incl - nb;
        const uint64_t x = v << (at & 31);
        if ((uint32_t)x) p.or_word(&s.out[at >> 5], (uint32_t)x);
        if (x >> 32) p.or_word(&s.out[(at >> 5) + 1], (uint32_t)(x >> 32));
      }
      base_bits += p.last(incl);
    }
    p.sync();
    if (lane == 0) {
      int pos = (int)base_bits;
      put_serial(s.out, &pos, s.code[256], s.len[256]);
      if (last) {
        s.out_len = (pos + 7) / 8;
      } else {
        const int at = (pos + 3 + 7) / 8;   // 000, zero bits to the boundary, 00 00 FF FF
        ob[at + 2] = 0xFF, ob[at + 3] = 0xFF;
        s.out_len = at + 4;
      }
    }
  } else {
    // the stored block
    if (lane == 0) {
      ob[0] = last ? 1 : 0;
      ob[1] = (uint8_t)(n & 255), ob[2] = (uint8_t)(n >> 8);
      ob[3] = (uint8_t)(~n & 255), ob[4] = (uint8_t)((~n >> 8) & 255);
      s.out_len = 5 + n;
    }
    for (int i = lane; i < n; i += L) ob[5 + i] = s.in[i];
  }
  p.sync();
  // 6. the CRC register over the bytes: every lane its own run of them, moved behind the others' by x^(8 bytes behind it)
  const int out_len = s.out_len;
  const int per = ((out_len + L - 1) / L + 3) & ~3;
  const int lo = lane * per < out_len ? lane * per : out_len, hi = lo + per < out_len ? lo + per : out_len;
  uint32_t c = 0;
  for (int i = lo; i < hi; ++i) c = s.crc_table[(c ^ ob[i]) & 255u] ^ (c >> 8);
  if (hi > lo && hi < out_len) c = multmodp(c, xpow_bytes(crc_pow, (uint64_t)(out_len - hi)));
  c = p.reduce_xor(c);
  // 7. to the staging area: whole dwords, the last bytes one by one (exactly out_len bytes are written)
  uint32_t* const sw = (uint32_t*)stage;
  for (int i = lane; i < out_len / 4; i += L) sw[i] = s.out[i];
  if (lane == 0) {
    for (int i = out_len & ~3; i < out_len; ++i) stage[i] = ob[i];
    rec->len = (uint32_t)out_len, rec->crc = c, rec->a = a, rec->b = b;
  }
}

// ---- a frame's checksums from its segments' (serial form: the assemble kernel does the same with 256 threads) ------------------
struct FrameSums {
  uint32_t crc_terms = 0, a = 0, b = 0;
};
// Adds segment s, `behind` coded bytes and `raw_behind` filtered bytes in front of the Adler-32 / the stream's end.
PR_PE_HD void add_segment(FrameSums& f, const SegRec& r, uint64_t behind, uint64_t raw_behind, const uint32_t* crc_pow) {
  f.crc_terms ^= multmodp(r.crc, xpow_bytes(crc_pow, behind + 4));
  f.a = (f.a + r.a) % kAdler;
  f.b = (uint32_t)((f.b + r.b + (uint64_t)r.a * (raw_behind % kAdler)) % kAdler);
}
PR_PE_HD uint32_t frame_adler(const FrameSums& f, uint64_t raw) {
  return ((uint32_t)((raw % kAdler + f.b) % kAdler) << 16) | ((1u + f.a) % kAdler);
}
// IDAT's CRC-32: `coded` bytes of segments between the zlib header and the Adler-32
PR_PE_HD uint32_t frame_idat_crc(const FrameSums& f, uint32_t head_state, uint64_t coded, uint32_t adler, const uint32_t* crc_pow) {
  uint32_t t = 0;
  for (int k = 3; k >= 0; --k) t = crc_byte(t, (adler >> (8 * k)) & 255u);
  return ~(multmodp(head_state, xpow_bytes(crc_pow, coded + 4)) ^ f.crc_terms ^ t);
}

}  // namespace pngenc
}  // namespace pr
