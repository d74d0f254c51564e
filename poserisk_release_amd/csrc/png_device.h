// The PNG decoder's device half written ONCE (include/poserisk_hip.h, section j4): the bit reader, the table construction, the
// symbol decode, every validation decision, the Adler-32 and the unfilter, templated on a small wave policy P:
//   PngWave64  64 lanes, cross-lane operations, LDS: what csrc/png.hip instantiates for gfx950;
//   PngLane1   one lane, plain C++: what tests/native/png_native.cc compiles with g++ under ASan + UBSan, so that the
//              same text that decides on the device is proven in-bounds on the host, on exact-size heap blocks.
// A policy supplies: L (lanes), lane(), uniform(x) (the value of the first lane: a hint that x is wave-uniform, so that the
// bit buffer lives in scalar registers), read_lane(v, k), ballot(pred), rank(mask) (set bits of mask below this lane),
// shfl_up1(v), table_sync() (LDS writes of the wave's other lanes are visible), stores_before_loads() (global stores of the
// wave's other lanes are visible to the loads that follow) and load_word(z, off, len) (the little-endian dword at byte `off`
// of a stream of `len` bytes; bytes at or behind `len` may hold anything and are masked off by the caller).
//
// What the 64-lane form does in parallel and the one-lane form therefore does not cover: the 64-wide literal and match
// stores, the ballot ranks of the table construction, the lane exchange of the unfilter.  tests/test_png_gpu.py (byte-exact
// cases, guard bands) covers those.
#pragma once
#include <cstdint>
#include <cstring>

#include "../../include/poserisk_hip.h"

#if defined(__HIPCC__)
#define PR_PNG_HD __host__ __device__ __forceinline__
#else
#define PR_PNG_HD inline
#endif

namespace pr {
namespace png {

constexpr int kLitRoot = 10, kDistRoot = 9, kCodesRoot = 7;   // first-level table bits; longer codes: canonical walk
constexpr int kMaxBits = 15;

// One set of decode tables: 4.1 KB.  A wave owns one for dynamic blocks; a workgroup shares one for fixed blocks.
struct Tables {
  uint16_t lit_fast[1 << kLitRoot];    // next 10 bits -> length << 9 | symbol for codes of <= 10 bits, else 0
  uint16_t dist_fast[1 << kDistRoot];  // next 9 bits likewise (the code-length code uses its first 128 entries while a header is read)
  uint16_t lit_sym[288];               // symbols in canonical order (by length, then by value)
  uint16_t dist_sym[32];
  uint16_t lit_cnt[16], dist_cnt[16];  // codes per length
  uint8_t lens[320];                   // the code lengths as the header gives them: HLIT literal/length, then HDIST distance
};

struct PngLane1 {
  static constexpr int L = 1;
  PR_PNG_HD int lane() const { return 0; }
  PR_PNG_HD uint32_t uniform(uint32_t v) const { return v; }
  PR_PNG_HD uint32_t read_lane(uint32_t v, int) const { return v; }
  PR_PNG_HD uint64_t ballot(bool p) const { return p ? 1u : 0u; }
  PR_PNG_HD int rank(uint64_t) const { return 0; }
  PR_PNG_HD uint32_t shfl_up1(uint32_t v) const { return v; }
  PR_PNG_HD void table_sync() const {}
  PR_PNG_HD void stores_before_loads() const {}
  PR_PNG_HD uint32_t load_word(const uint8_t* z, int64_t off, int64_t len) const {   // exact-size blocks: never past len
    uint32_t w = 0;
    const int64_t n = len - off < 4 ? len - off : 4;
    for (int64_t i = 0; i < n; ++i) w |= (uint32_t)z[off + i] << (8 * i);
    return w;
  }
};

// ---- bit reader: LSB-first, a 64-bit buffer that only ever holds bits of the stream -------------------------------------
template <class P>
struct Bits {
  const uint8_t* z;
  int64_t len;     // the stream's length: no bit behind it exists
  int64_t next;    // the first byte not yet in `hold`
  uint64_t hold;
  int nbits;
  int64_t cw;      // the dword index this wave's chunk starts at (lane i holds dword cw + i), -1 before the first load
  uint32_t word;

  PR_PNG_HD void init(const uint8_t* z_, int64_t len_, int64_t at) {
    z = z_;
    len = len_;
    next = at;
    hold = 0;
    nbits = 0;
    cw = -1;
    word = 0;
  }
  // Tops the buffer up to more than 32 bits, or to the stream's end.  A refill reads whole dwords inside the stream; the bytes
  // of the last dword behind `len` are masked off, so `hold` never holds a bit that is not the stream's.
  PR_PNG_HD void refill(const P& p) {
    while (nbits <= 32 && next < len) {
      const int64_t wi = next >> 2;
      if (cw < 0 || wi < cw || wi >= cw + P::L) {
        cw = wi;
        const int64_t mine = (wi + p.lane()) * 4;
        word = mine < len ? p.load_word(z, mine, len) : 0u;
      }
      uint32_t w = p.read_lane(word, (int)(wi - cw));
      const int sh = (int)(next & 3) * 8;
      w >>= sh;
      int nb = 32 - sh;
      const int64_t left = len - next;
      if (left * 8 < nb) {
        nb = (int)left * 8;
        w &= (1u << nb) - 1u;
      }
      hold |= (uint64_t)w << nbits;
      nbits += nb;
      next += nb >> 3;
    }
  }
  PR_PNG_HD void drop(int n) {
    hold >>= n;
    nbits -= n;
  }
  // n <= 16 bits; false (nothing consumed) when the stream has fewer left
  PR_PNG_HD bool take(int n, uint32_t* v) {
    if (n > nbits) return false;
    *v = (uint32_t)hold & ((1u << n) - 1u);
    drop(n);
    return true;
  }
  PR_PNG_HD int64_t byte_pos() const { return next - (nbits >> 3); }   // valid when nbits is a multiple of 8
};

enum { kOk = 0, kBadCode = -1, kTruncated = -2 };

// The canonical walk (one bit a length) on `bits`, for code lengths 1..max_len: the symbol's index in canonical order and
// its length, or -1.
PR_PNG_HD int walk(uint64_t bits, const uint16_t* cnt, int max_len, int* length) {
  int code = 0, first = 0, index = 0;
  for (int l = 1; l <= max_len; ++l) {
    code |= (int)(bits & 1);
    bits >>= 1;
    const int c = cnt[l];
    if (code - c < first) {
      *length = l;
      return index + (code - first);
    }
    index += c;
    first += c;
    first <<= 1;
    code <<= 1;
  }
  return -1;
}

// One symbol: >= 0, or kBadCode (no code of the set matches the bits) or kTruncated (the matching code, or any code that
// could still match, needs bits behind the stream's end).
template <class P>
PR_PNG_HD int decode(const P& p, Bits<P>& b, const uint16_t* fast, int root, const uint16_t* cnt, const uint16_t* sym) {
  const uint32_t e = p.uniform(fast[(uint32_t)b.hold & ((1u << root) - 1u)]);
  if (e) {
    const int l = (int)(e >> 9);
    if (l > b.nbits) return kTruncated;
    b.drop(l);
    return (int)(e & 511u);
  }
  int code = 0, first = 0, index = 0;
  uint64_t bits = b.hold;
  for (int l = 1; l <= kMaxBits; ++l) {
    code |= (int)(bits & 1);
    bits >>= 1;
    const int c = (int)p.uniform(cnt[l]);
    if (code - c < first) {
      if (l > b.nbits) return kTruncated;
      b.drop(l);
      return (int)p.uniform(sym[index + (code - first)]);
    }
    index += c;
    first += c;
    first <<= 1;
    code <<= 1;
  }
  return b.nbits < kMaxBits ? kTruncated : kBadCode;
}

enum { kCodes = 0, kLens = 1, kDists = 2 };

// Builds cnt / sym / fast from n code lengths, all lanes together: the lanes count and rank 64 symbols at a time by
// ballot, then fill the first-level table, each lane the entries lane, lane + L, ... by the canonical walk.  zlib's rules:
// over-subscribed is an error; incomplete is an error for the code-length code and otherwise unless the set is one code of
// length 1; no code at all is legal for a distance set (every entry stays 0: any use is a bad code).
template <class P>
PR_PNG_HD bool build(const P& p, const uint8_t* lens, int n, int kind, int root, uint16_t* cnt, uint16_t* sym, uint16_t* fast) {
  int c[kMaxBits + 1];
#pragma unroll
  for (int l = 0; l <= kMaxBits; ++l) c[l] = 0;
  for (int s0 = 0; s0 < n; s0 += P::L) {
    const int s = s0 + p.lane();
    const int mine = s < n ? lens[s] : 0;
#pragma unroll
    for (int l = 1; l <= kMaxBits; ++l) c[l] += __builtin_popcountll(p.ballot(mine == l));
  }
  int left = 1, max_len = 0;
#pragma unroll
  for (int l = 1; l <= kMaxBits; ++l) {
    left = left * 2 - c[l];
    if (left < 0) return false;                                    // over-subscribed
    if (c[l]) max_len = l;
  }
  if (max_len == 0) {
    if (kind != kDists) return false;
  } else if (left > 0 && (kind == kCodes || max_len != 1)) {
    return false;                                                  // incomplete
  }
  int offs[kMaxBits + 1];
  offs[0] = 0;
  offs[1] = 0;
#pragma unroll
  for (int l = 1; l < kMaxBits; ++l) offs[l + 1] = offs[l] + c[l];
  cnt[0] = 0;
#pragma unroll
  for (int l = 1; l <= kMaxBits; ++l) cnt[l] = (uint16_t)c[l];     // every lane the same value
  for (int s0 = 0; s0 < n; s0 += P::L) {
    const int s = s0 + p.lane();
    const int mine = s < n ? lens[s] : 0;
#pragma unroll
    for (int l = 1; l <= kMaxBits; ++l) {
      const uint64_t m = p.ballot(mine == l);
      if (mine == l) sym[offs[l] + p.rank(m)] = (uint16_t)s;
      offs[l] += __builtin_popcountll(m);
    }
  }
  p.table_sync();
  for (int e = p.lane(); e < (1 << root); e += P::L) {
    int l = 0;
    const int i = walk((uint64_t)e, cnt, root < max_len ? root : max_len, &l);
    fast[e] = i < 0 ? (uint16_t)0 : (uint16_t)(l << 9 | sym[i]);
  }
  p.table_sync();
  return true;
}

// The fixed block's tables (RFC 1951 3.2.6): 288 literal/length codes of 8, 9, 7, 8 bits and 32 distance codes of 5.  Symbols
// 286, 287 and distances 30, 31 have codes and are refused where they are decoded.
template <class P>
PR_PNG_HD void build_fixed(const P& p, Tables* t) {
  for (int s = p.lane(); s < 320; s += P::L) t->lens[s] = (uint8_t)(s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : s < 288 ? 8 : 5);
  p.table_sync();
  build(p, t->lens, 288, kLens, kLitRoot, t->lit_cnt, t->lit_sym, t->lit_fast);
  build(p, t->lens + 288, 32, kDists, kDistRoot, t->dist_cnt, t->dist_sym, t->dist_fast);
}

// A dynamic block's header (RFC 1951 3.2.7) into t: 0, or PR_PNG_ST_TRUNCATED / PR_PNG_ST_BAD_CODE.
template <class P>
PR_PNG_HD int read_dynamic(const P& p, Bits<P>& b, Tables* t) {
  const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
  uint32_t v = 0;
  b.refill(p);
  if (!b.take(14, &v)) return PR_PNG_ST_TRUNCATED;
  const int hlit = (int)(v & 31) + 257, hdist = (int)(v >> 5 & 31) + 1, hclen = (int)(v >> 10) + 4;
  if (hlit > 286 || hdist > 30) return PR_PNG_ST_BAD_CODE;
  for (int i = p.lane(); i < 19; i += P::L) t->lens[i] = 0;
  p.table_sync();
  for (int i = 0; i < hclen; ++i) {
    b.refill(p);
    if (!b.take(3, &v)) return PR_PNG_ST_TRUNCATED;
    t->lens[order[i]] = (uint8_t)v;                                // every lane the same value
  }
  p.table_sync();
  if (!build(p, t->lens, 19, kCodes, kCodesRoot, t->dist_cnt, t->dist_sym, t->dist_fast)) return PR_PNG_ST_BAD_CODE;
  const int total = hlit + hdist;
  int have = 0, prev = 0;
  while (have < total) {
    b.refill(p);
    const int s = decode(p, b, t->dist_fast, kCodesRoot, t->dist_cnt, t->dist_sym);
    if (s < 0) return s == kTruncated ? PR_PNG_ST_TRUNCATED : PR_PNG_ST_BAD_CODE;
    if (s < 16) {
      t->lens[have++] = (uint8_t)s;
      prev = s;
      continue;
    }
    int rep = 0, val = 0;
    if (s == 16) {
      if (have == 0) return PR_PNG_ST_BAD_CODE;
      if (!b.take(2, &v)) return PR_PNG_ST_TRUNCATED;
      rep = 3 + (int)v;
      val = prev;
    } else if (s == 17) {
      if (!b.take(3, &v)) return PR_PNG_ST_TRUNCATED;
      rep = 3 + (int)v;
    } else {
      if (!b.take(7, &v)) return PR_PNG_ST_TRUNCATED;
      rep = 11 + (int)v;
    }
    if (have + rep > total) return PR_PNG_ST_BAD_CODE;
    for (int i = p.lane(); i < rep; i += P::L) t->lens[have + i] = (uint8_t)val;
    have += rep;
    prev = val;
  }
  p.table_sync();
  if (t->lens[256] == 0) return PR_PNG_ST_BAD_CODE;               // no end-of-block code
  if (!build(p, t->lens, hlit, kLens, kLitRoot, t->lit_cnt, t->lit_sym, t->lit_fast)) return PR_PNG_ST_BAD_CODE;
  if (!build(p, t->lens + hlit, hdist, kDists, kDistRoot, t->dist_cnt, t->dist_sym, t->dist_fast)) return PR_PNG_ST_BAD_CODE;
  return 0;
}

// What a caller may want to know about a stream it inflated (tests/test_png_native.py reads it; the kernel passes nullptr).
struct InflateStats {
  int64_t blocks[3], literals, matches;
};

// Inflates the zlib stream z[skew, skew + zlen) (header already validated by the parser: two bytes are skipped) into
// out[0, raw): returns 0 or PR_PNG_ST_* bits and, with 0, the trailer's Adler-32 in *adler.  z is where the reader's dwords are
// counted from (the device passes the 16-byte line the stream starts in, skew = 0..15; bytes in front of skew may be loaded
// with the stream's first dword and are shifted out).  Every read of z is bounded by skew + zlen, every write of out by raw, every match reads out below the position it writes.  `dyn` is this wave's own table set, `fixed`
// the shared one (build_fixed).
template <class P>
PR_PNG_HD int inflate(const P& p, const uint8_t* z, int64_t skew, int64_t zlen, uint8_t* out, int64_t raw, Tables* dyn, const Tables* fixed,
                      uint32_t* adler, InflateStats* stats) {
  const uint16_t len_base[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
  const uint8_t len_extra[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
  const uint16_t dist_base[30] = {1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097,
                                  6145, 8193, 12289, 16385, 24577};
  const uint8_t dist_extra[30] = {0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13};
  if (zlen < 2) return PR_PNG_ST_TRUNCATED;
  const int64_t zend = skew + zlen;
  Bits<P> b;
  b.init(z, zend, skew + 2);
  int64_t pos = 0;          // bytes of out written (the pending literals not counted)
  int nl = 0;               // pending literals: lane i holds the i-th
  uint32_t mylit = 0;
  int64_t unsynced = -1;    // the lowest position stored since the last stores_before_loads(), -1 when none
  uint32_t v = 0;
  auto flush = [&]() {
    if (nl) {
      if (p.lane() < nl) out[pos + p.lane()] = (uint8_t)mylit;
      if (unsynced < 0) unsynced = pos;
      pos += nl;
      nl = 0;
    }
  };
  for (;;) {
    b.refill(p);
    if (!b.take(3, &v)) return PR_PNG_ST_TRUNCATED;
    const int final_block = (int)(v & 1), type = (int)(v >> 1);
    if (type == 3) return PR_PNG_ST_BAD_CODE;
    if (stats) ++stats->blocks[type];
    if (type == 0) {
      flush();
      b.drop(b.nbits & 7);
      b.refill(p);
      if (b.nbits < 32) return PR_PNG_ST_TRUNCATED;
      const uint32_t ln = (uint32_t)b.hold & 0xFFFFu, nln = (uint32_t)(b.hold >> 16) & 0xFFFFu;
      if (ln != (nln ^ 0xFFFFu)) return PR_PNG_ST_BAD_CODE;
      b.drop(32);
      const int64_t at = b.byte_pos();
      if (at + (int64_t)ln > zend) return PR_PNG_ST_TRUNCATED;
      if (pos + (int64_t)ln > raw) return PR_PNG_ST_SIZE;
      for (int64_t j = p.lane(); j < (int64_t)ln; j += P::L) out[pos + j] = z[at + j];
      if (ln && unsynced < 0) unsynced = pos;
      pos += ln;
      b.next = at + ln;                                            // the reader goes on behind the copied bytes
      b.hold = 0;
      b.nbits = 0;
    } else {
      const Tables* t = fixed;
      if (type == 2) {
        const int st = read_dynamic(p, b, dyn);
        if (st) return st;
        t = dyn;
      }
      for (;;) {
        b.refill(p);
        const int s = decode(p, b, t->lit_fast, kLitRoot, t->lit_cnt, t->lit_sym);
        if (s < 0) return s == kTruncated ? PR_PNG_ST_TRUNCATED : PR_PNG_ST_BAD_CODE;
        if (s < 256) {
          if (pos + nl >= raw) return PR_PNG_ST_SIZE;
          if (p.lane() == nl) mylit = (uint32_t)s;
          if (++nl == P::L) flush();
          if (stats) ++stats->literals;
          continue;
        }
        if (s == 256) break;
        if (s > 285) return PR_PNG_ST_BAD_CODE;
        int length = len_base[s - 257];
        if (!b.take(len_extra[s - 257], &v)) return PR_PNG_ST_TRUNCATED;
        length += (int)v;
        b.refill(p);
        const int d = decode(p, b, t->dist_fast, kDistRoot, t->dist_cnt, t->dist_sym);
        if (d < 0) return d == kTruncated ? PR_PNG_ST_TRUNCATED : PR_PNG_ST_BAD_CODE;
        if (d > 29) return PR_PNG_ST_BAD_CODE;
        if (!b.take(dist_extra[d], &v)) return PR_PNG_ST_TRUNCATED;
        const int64_t dist = dist_base[d] + (int64_t)v;
        if (dist > pos + nl) return PR_PNG_ST_BAD_CODE;            // reaches before the start of the output
        flush();
        if (pos + length > raw) return PR_PNG_ST_SIZE;
        const int64_t src = pos - dist;
        const int64_t span = dist < length ? dist : length;        // the bytes read: out[src, src + span), all below pos
        if (unsynced >= 0 && src + span > unsynced) {
          p.stores_before_loads();
          unsynced = -1;
        }
        if (dist >= length) {
          for (int j = p.lane(); j < length; j += P::L) out[pos + j] = out[src + j];
        } else {
          // an overlapping run: byte j of the match is byte j mod dist of the period in front of it, which is complete
          for (int j = p.lane(); j < length; j += P::L) out[pos + j] = out[src + j % (int)dist];
        }
        if (unsynced < 0) unsynced = pos;
        pos += length;
        if (stats) ++stats->matches;
      }
    }
    if (final_block) break;
  }
  flush();
  b.drop(b.nbits & 7);
  b.refill(p);
  if (b.nbits < 32) return PR_PNG_ST_TRUNCATED;
  const uint32_t h = (uint32_t)b.hold;
  *adler = (h & 255u) << 24 | (h >> 8 & 255u) << 16 | (h >> 16 & 255u) << 8 | h >> 24;
  return pos == raw ? 0 : PR_PNG_ST_SIZE;
}

// ---- Adler-32 ----------------------------------------------------------------------------------------------------------
// A = 1 + sum b_k, B = n + sum (n - k) b_k (mod 65521), k from 0.  Thread t of T takes bytes t, t + T, ...: its partial sums
// s1 = sum b_k and s2 = sum k b_k (k < 2^27, at most 2^19 bytes a thread at T = 256: below 2^54) combine as
// B = n + n s1 - s2.  Returns the thread's (s1 mod 65521, s2 mod 65521).
PR_PNG_HD void adler_partial(const uint8_t* raw, int64_t n, int t, int T, uint32_t* s1, uint32_t* s2) {
  uint64_t a = 0, w = 0;
  for (int64_t k = t; k < n; k += T) {
    a += raw[k];
    w += (uint64_t)k * raw[k];
  }
  *s1 = (uint32_t)(a % 65521u);
  *s2 = (uint32_t)(w % 65521u);
}
PR_PNG_HD uint32_t adler_combine(uint64_t s1, uint64_t s2, int64_t n) {   // s1, s2: sums of the partials (each below 2^40)
  s1 %= 65521u;
  s2 %= 65521u;
  const uint64_t nm = (uint64_t)n % 65521u;
  const uint32_t A = (uint32_t)((1 + s1) % 65521u);
  const uint32_t B = (uint32_t)((nm + nm * s1 + 65521u - s2) % 65521u);
  return B << 16 | A;
}

// ---- unfilter ----------------------------------------------------------------------------------------------------------
PR_PNG_HD uint32_t paeth(int a, int b, int c) {
  const int pp = a + b - c;
  const int pa = pp > a ? pp - a : a - pp, pb = pp > b ? pp - b : b - pp, pc = pp > c ? pp - c : c - pp;
  return (uint32_t)((pa <= pb && pa <= pc) ? a : pb <= pc ? b : c);
}
// One pixel (bpp bytes packed little-endian in a dword): x the filtered bytes, a / b / c the unfiltered neighbours.
PR_PNG_HD uint32_t unfilter_pixel(int ft, int bpp, uint32_t x, uint32_t a, uint32_t b, uint32_t c) {
  uint32_t r = 0;
  for (int i = 0; i < bpp; ++i) {
    const int sh = 8 * i;
    const int xi = (int)(x >> sh & 255u), ai = (int)(a >> sh & 255u), bi = (int)(b >> sh & 255u), ci = (int)(c >> sh & 255u);
    const uint32_t pred = ft == 1 ? (uint32_t)ai : ft == 2 ? (uint32_t)bi : ft == 3 ? (uint32_t)((ai + bi) >> 1) : ft == 4 ? paeth(ai, bi, ci) : 0u;
    r |= (((uint32_t)xi + pred) & 255u) << sh;
  }
  return r;
}
PR_PNG_HD uint32_t load_pixel(const uint8_t* q, int bpp) {
  uint32_t v = 0;
  for (int i = 0; i < bpp; ++i) v |= (uint32_t)q[i] << (8 * i);
  return v;
}

// Undoes the filters of rows [r0, r0 + P::L) of raw (H rows of 1 + W bpp bytes) in place; rows below r0 are done.  Lane l takes
// row r0 + l and runs one pixel behind lane l - 1: at step t it is at pixel t - l, its upper neighbour b is what lane l - 1
// produced one step earlier (shfl_up1), its upper-left c the b of its own previous step.  Lane 0 reads the row above from
// memory.  Returns true when a filter byte of these rows is above 4 (such a row is taken as filter 0).
template <class P>
PR_PNG_HD bool unfilter_pass(const P& p, uint8_t* raw, int H, int W, int bpp, int r0) {
  const int64_t stride = 1 + (int64_t)W * bpp;
  const int row = r0 + p.lane();
  const bool live = row < H;
  uint8_t* mine = raw + (live ? row : 0) * stride;
  int ft = live ? mine[0] : 0;
  const bool bad = ft > 4;
  if (bad) ft = 0;
  const uint8_t* above = r0 > 0 ? raw + (int64_t)(r0 - 1) * stride + 1 : nullptr;
  uint32_t cur = 0, a = 0, c = 0;
  const int rows = H - r0 < P::L ? H - r0 : P::L;
  for (int t = 0; t < W + rows - 1; ++t) {
    uint32_t b = p.shfl_up1(cur);                                  // every lane takes part, also the idle ones
    const int x = t - p.lane();
    if (p.lane() == 0) b = (above && x < W) ? load_pixel(above + (int64_t)x * bpp, bpp) : 0u;
    if (live && x >= 0 && x < W) {
      if (x == 0) a = c = 0;
      uint8_t* q = mine + 1 + (int64_t)x * bpp;
      cur = unfilter_pixel(ft, bpp, load_pixel(q, bpp), a, b, c);
      for (int i = 0; i < bpp; ++i) q[i] = (uint8_t)(cur >> (8 * i));
      a = cur;
    }
    c = b;
  }
  return p.ballot(bad) != 0;
}

// true when row r (> 0) needs nothing of the row above: its filter is None or Sub (or invalid, taken as None)
PR_PNG_HD bool row_independent(const uint8_t* raw, int64_t stride, int r) {
  const int ft = raw[(int64_t)r * stride];
  return ft == 0 || ft == 1 || ft > 4;
}

PR_PNG_HD void colour_pixel(int color_type, int bpp, const uint8_t* q, const uint8_t* palette, int bgr, uint8_t* rgb) {
  uint8_t r, g, bl;
  if (color_type == 3) {
    const uint8_t* e = palette + 3 * (int)q[0];
    r = e[0], g = e[1], bl = e[2];
  } else if (bpp >= 3) {
    r = q[0], g = q[1], bl = q[2];
  } else {
    r = g = bl = q[0];
  }
  rgb[0] = bgr ? bl : r;
  rgb[1] = g;
  rgb[2] = bgr ? r : bl;
}

// The checks every kernel makes of a frame's descriptor before it forms an address from it.
PR_PNG_HD bool frame_ok(const pr_png_frame& fr, const pr_png_args& a) {
  const int want = fr.color_type == 0 ? 1 : fr.color_type == 2 ? 3 : fr.color_type == 3 ? 1 : fr.color_type == 4 ? 2 : fr.color_type == 6 ? 4 : -1;
  if (fr.bpp != want || fr.width != a.W || fr.height != a.H) return false;
  if (fr.n_idat < 1 || fr.first_idat < 0 || fr.first_idat > a.n_idat - fr.n_idat) return false;
  if (fr.color_type == 3 && (fr.palette < 0 || fr.palette >= a.n_palettes)) return false;
  return fr.zlib_bytes >= 2 && fr.zlib_bytes <= a.data_bytes;
}

}  // namespace png
}  // namespace pr
