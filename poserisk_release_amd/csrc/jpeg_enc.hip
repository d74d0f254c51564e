// Device half of the JPEG encoder: u8 frames on the device -> complete baseline JPEG files in per-frame slots.  The contract --
// the arithmetic, the 32-bit FDCT bound, the capacity rule -- is written in include/poserisk_hip.h (section j2);
// tests/jpeg_enc_ref.py restates it in numpy, tests/test_jpeg_encode_native.py runs this file on the host under sanitizers and
// tests/test_jpeg_encode_gpu.py compares every byte with libjpeg's.  Blocks are numbered in scan order: b = MCU * bpm + k, the
// MCU's luma blocks first (row-major), then Cb, then Cr.
//
//   transform  one lane per 8x8 block: colour conversion, edge replication, chroma downsampling, FDCT (32-bit), quantisation by
//              reciprocal; int16 coefficients in zig-zag order, and one word per block: AC bit count, DC term, dummy flag.
//   scan       one lane per restart segment, serial over its blocks' words: dummy blocks take the previous block's DC, DC
//              differences per component, each block's bit offset inside the segment, the segment's bit count.
//   layout     one lane per frame: the segments' places (whole 64-byte chunks) in the frame's unstuffed buffer; a frame whose
//              unstuffed data already exceeds its slot is marked as overflowing and skipped from here on.
//   emit       one lane per block: its Huffman codes at its bit offset into the zeroed unstuffed buffer, most significant bit
//              first inside 32-bit words.  A word two blocks share is combined with atomicOr, words in between are stored.
//              A segment's last block adds the pad bits.
//   count      one lane per 64-byte chunk: its 0xFF bytes.   prefix: one lane per segment over its chunks' counts.
//   size       one lane per frame: the segments' places in the slot; nbytes, or overflow.
//   place      one lane per chunk (and ten per frame for the header): the final bytes with the stuffed zeros, RSTn / EOI behind
//              a segment's last chunk.
// Kernels index by thread only: no LDS, no barrier, no cross-lane operation, plain C++ and vector memory operations.
#include "common.h"

namespace pr {
namespace {

constexpr int kEncThreads = 256;
constexpr int kChunk = 64;                                       // bytes of unstuffed data one count / place lane handles
constexpr int kChunkWords = kChunk / 4;
constexpr int kHeaderLanes = PR_JPEG_ENC_HEADER_MAX / kChunk;    // lanes of `place` that copy the header

// zig-zag position -> natural index.  constexpr, so that the unrolled loops of the transform index registers by constants
constexpr unsigned char kEncZigzag[64] = {
    0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28,
    35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

struct EncParams {
  pr_jpeg_enc_args a;
  int mx, my, nl, bpm;     // MCUs across and down, luma blocks and all blocks per MCU
  int nmcu, nb;            // MCUs and blocks per frame
  int ri, nseg;            // MCUs per restart segment (nmcu where there is no interval), segments per frame
  int rbw, rbh;            // luma's own blocks across and down: ceil(W / 8), ceil(H / 8); beyond them blocks are dummies
  int U;                   // chunks of unstuffed data a frame has room for
  unsigned* bits;          // [F][U][16]  unstuffed segment data, big-endian bit order inside each word
  short* coef;             // [F][nb][64] zig-zag order
  int* info;               // [F][nb]     transform: dummy << 31 | AC bits << 16 | DC & 0xffff;  scan: bit offset in the segment
  int* seg_bits;           // [F][nseg]
  int* seg_chunk;          // [F][nseg+1] first chunk of each segment in the frame's unstuffed buffer
  int* seg_out;            // [F][nseg]   prefix: the segment's stuffed size;  size: its byte offset in the slot
  int* ff;                 // [F][U]      count: 0xFF bytes of the chunk;  prefix: those of the segment's earlier chunks
  int* fstate;             // [F]         1 = the frame does not fit its slot
  short* diff;             // [F][nb]     DC differences
};

__device__ __forceinline__ int bit_length(int magnitude) { return magnitude ? 32 - __builtin_clz((unsigned)magnitude) : 0; }

__device__ __forceinline__ int enc_descale(unsigned x, int n) { return (int)(x + (1u << (n - 1))) >> n; }

// One 1-D pass of jfdctint.c on d[0], d[s], ..., d[7 s], in place; 32-bit ring arithmetic (section j2).
template <bool kFirst>
__device__ __forceinline__ void fdct_pass(int* d, int s) {
  const unsigned d0 = (unsigned)d[0], d1 = (unsigned)d[s], d2 = (unsigned)d[2 * s], d3 = (unsigned)d[3 * s], d4 = (unsigned)d[4 * s],
                 d5 = (unsigned)d[5 * s], d6 = (unsigned)d[6 * s], d7 = (unsigned)d[7 * s];
  unsigned t0 = d0 + d7, t7 = d0 - d7, t1 = d1 + d6, t6 = d1 - d6, t2 = d2 + d5, t5 = d2 - d5, t3 = d3 + d4, t4 = d3 - d4;
  const unsigned t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  constexpr int n = kFirst ? 11 : 15;
  d[0] = kFirst ? (int)((t10 + t11) << 2) : enc_descale(t10 + t11, 2);
  d[4 * s] = kFirst ? (int)((t10 - t11) << 2) : enc_descale(t10 - t11, 2);
  unsigned z1 = (t12 + t13) * 4433u;
  d[2 * s] = enc_descale(z1 + t13 * 6270u, n);
  d[6 * s] = enc_descale(z1 - t12 * 15137u, n);
  z1 = t4 + t7;
  unsigned z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
  const unsigned z5 = (z3 + z4) * 9633u;
  t4 *= 2446u;
  t5 *= 16819u;
  t6 *= 25172u;
  t7 *= 12299u;
  z1 *= (unsigned)-7373;
  z2 *= (unsigned)-20995;
  z3 = z3 * (unsigned)-16069 + z5;
  z4 = z4 * (unsigned)-3196 + z5;
  d[7 * s] = enc_descale(t4 + z1 + z3, n);
  d[5 * s] = enc_descale(t5 + z2 + z4, n);
  d[3 * s] = enc_descale(t6 + z2 + z3, n);
  d[s] = enc_descale(t7 + z1 + z4, n);
}

// samples - 128 (natural order) -> coefficients scaled by 8, in place
__device__ __forceinline__ void fdct8x8(int* d) {
#pragma unroll
  for (int r = 0; r < 8; ++r) fdct_pass<true>(d + 8 * r, 1);
#pragma unroll
  for (int c = 0; c < 8; ++c) fdct_pass<false>(d + c, 8);
}

// (|c| + q8 / 2) / q8 with the sign restored, by the reciprocal ceil(2^32 / q8): exact for |c| + q8 / 2 < 2^21
__device__ __forceinline__ int enc_quantise(int c, unsigned q8, unsigned recip) {
  const unsigned x = (unsigned)(c < 0 ? -c : c) + (q8 >> 1);
  const int m = (int)(((unsigned long long)x * recip) >> 32);
  return c < 0 ? -m : m;
}

struct Ycc {
  int y, cb, cr;
};

__device__ __forceinline__ Ycc load_ycc(const unsigned char* px, int bgr) {
  const int c0 = px[0], G = px[1], c2 = px[2];
  const int R = bgr ? c2 : c0, B = bgr ? c0 : c2;
  Ycc o;
  o.y = (19595 * R + 38470 * G + 7471 * B + 32768) >> 16;
  o.cb = (-11059 * R - 21709 * G + 32768 * B + (128 << 16) + 32767) >> 16;
  o.cr = (32768 * R - 27439 * G - 5329 * B + (128 << 16) + 32767) >> 16;
  return o;
}

__device__ __forceinline__ int pick(const Ycc& v, int comp) { return comp == 0 ? v.y : comp == 1 ? v.cb : v.cr; }

// ---- transform --------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kEncThreads) jpeg_enc_transform_kernel(EncParams p) {
  const pr_jpeg_enc_args& a = p.a;
  const int b = (int)(blockIdx.x * kEncThreads + threadIdx.x), f = (int)blockIdx.y;
  if (b >= p.nb) return;
  const int mcu = b / p.bpm, k = b - mcu * p.bpm;
  const int mr = mcu / p.mx, mc = mcu - mr * p.mx;
  const int comp = k < p.nl ? 0 : k - p.nl + 1;
  const int by = comp ? mr : mr * a.vs + k / a.hs, bx = comp ? mc : mc * a.hs + k % a.hs;
  const bool dummy = comp == 0 && (by >= p.rbh || bx >= p.rbw);
  const pr_jpeg_enc_plan& plan = *a.plan;
  const int t = comp ? 1 : 0;
  short* dst = p.coef + ((long)f * p.nb + b) * 64;
  int* info = p.info + (long)f * p.nb + b;
  if (dummy) {   // AC terms zero; the DC term is the previous block's (scan)
    for (int i = 0; i < 64; ++i) dst[i] = 0;
    *info = (int)(0x80000000u | ((unsigned)plan.ac_len[0][0] << 16));
    return;
  }
  const unsigned char* frame = a.frames + (long)f * a.H * a.W * 3;
  const int H = a.H, W = a.W;
  int d[64];
  // One rule for every component (section j2): a sample is the biased mean of sx x sy source pixels; the sample row is clamped
  // to the component's last own row first, then every source row and column to the image.
  const int sx = comp ? a.hs : 1, sy = comp ? a.vs : 1;
  const int last_row = (H + sy - 1) / sy - 1;
  const int shift = sx * sy == 4 ? 2 : sx * sy == 2 ? 1 : 0;
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    const int yr = min(by * 8 + r, last_row);
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      const int xc = bx * 8 + c;
      int sum = shift == 2 ? 1 + (c & 1) : shift == 1 ? (c & 1) : 0;   // h2v2: 1, 2, 1, 2, ...; h2v1: 0, 1, 0, 1, ...
      for (int dy = 0; dy < sy; ++dy) {
        const unsigned char* row = frame + (long)min(yr * sy + dy, H - 1) * W * 3;
        for (int dx = 0; dx < sx; ++dx) sum += pick(load_ycc(row + min(xc * sx + dx, W - 1) * 3, a.bgr), comp);
      }
      d[r * 8 + c] = (sum >> shift) - 128;
    }
  }
  fdct8x8(d);
#pragma unroll
  for (int i = 0; i < 64; ++i) d[i] = enc_quantise(d[i], 8u * plan.quant[t][i], plan.recip[t][i]);
  int bits = 0, run = 0;
#pragma unroll
  for (int z0 = 0; z0 < 64; z0 += 8) {   // eight coefficients = one 16-byte store
    unsigned packed[4];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int z = z0 + j;
      const int v = d[kEncZigzag[z]];
      if (j & 1) packed[j >> 1] |= (unsigned)v << 16;
      else packed[j >> 1] = (unsigned)v & 0xffffu;
      if (z == 0) continue;
      if (v == 0) {
        ++run;
      } else {
        const int n = bit_length(v < 0 ? -v : v);
        bits += (run >> 4) * plan.ac_len[t][0xF0] + plan.ac_len[t][(run & 15) << 4 | n] + n;
        run = 0;
      }
    }
    __builtin_memcpy(__builtin_assume_aligned(dst + z0, 16), packed, 16);
  }
  if (run) bits += plan.ac_len[t][0];
  *info = (int)(((unsigned)bits << 16) | ((unsigned)d[0] & 0xffffu));
}

// ---- scan -------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kEncThreads) jpeg_enc_scan_kernel(EncParams p) {
  const long i = (long)blockIdx.x * kEncThreads + threadIdx.x;
  if (i >= (long)p.a.F * p.nseg) return;
  const int f = (int)(i / p.nseg), s = (int)(i - (long)f * p.nseg);
  const pr_jpeg_enc_plan& plan = *p.a.plan;
  const int m0 = s * p.ri, m1 = min(m0 + p.ri, p.nmcu);
  int* info = p.info + (long)f * p.nb;
  short* diff = p.diff + (long)f * p.nb;
  int pred0 = 0, pred1 = 0, pred2 = 0, prev = 0, pos = 0;
  for (int m = m0; m < m1; ++m)
    for (int k = 0; k < p.bpm; ++k) {
      const int b = m * p.bpm + k;
      const int w = info[b];
      const int dc = w < 0 ? prev : (int)(short)(w & 0xffff);
      prev = dc;
      const int comp = k < p.nl ? 0 : k - p.nl + 1;
      const int pred = comp == 0 ? pred0 : comp == 1 ? pred1 : pred2;
      const int dd = dc - pred;
      if (comp == 0) pred0 = dc;
      else if (comp == 1) pred1 = dc;
      else pred2 = dc;
      const int n = bit_length(dd < 0 ? -dd : dd);
      diff[b] = (short)dd;
      info[b] = pos;
      pos += plan.dc_len[comp ? 1 : 0][n] + n + ((w >> 16) & 0x7fff);
    }
  p.seg_bits[i] = pos;
}

// ---- layout -----------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kEncThreads) jpeg_enc_layout_kernel(EncParams p) {
  const int f = (int)(blockIdx.x * kEncThreads + threadIdx.x);
  if (f >= p.a.F) return;
  const int* seg_bits = p.seg_bits + (long)f * p.nseg;
  int* seg_chunk = p.seg_chunk + (long)f * (p.nseg + 1);
  long c = 0;
  bool fits = true;
  for (int s = 0; s < p.nseg; ++s) {
    seg_chunk[s] = (int)c;
    c += (seg_bits[s] + 8 * kChunk - 1) / (8 * kChunk);
    if (c > p.U) {   // more unstuffed data than the slot holds bytes: the file cannot fit
      fits = false;
      break;
    }
  }
  seg_chunk[p.nseg] = (int)c;
  p.fstate[f] = fits ? 0 : 1;
  p.a.status[f] = fits ? 0 : (int)PR_JPEG_ENC_ST_OVERFLOW;
  p.a.nbytes[f] = 0;
}

// ---- emit -------------------------------------------------------------------------------------------------------------------
// Bits go into 32-bit words most significant bit first.  `cur` collects the word at index `word`, `fill` of its bits are
// taken (by this block or by those in front of it).  The first word a block touches and the word it leaves unfinished may be
// shared with its neighbours in the segment: those are combined with atomicOr over the zeroed buffer, the others stored.
struct BitWriter {
  unsigned* words;
  long word;
  unsigned cur;
  int fill;
  bool first;
};

__device__ __forceinline__ void flush_word(BitWriter& w) {
  if (w.first) atomicOr((int*)(w.words + w.word), (int)w.cur);
  else w.words[w.word] = w.cur;
  w.first = false;
  ++w.word;
  w.cur = 0u;
}

__device__ __forceinline__ void put_bits(BitWriter& w, unsigned code, int len) {   // 1 <= len <= 16, code < 2^len
  const int end = w.fill + len;
  if (end <= 32) {
    w.cur |= code << (32 - end);
    w.fill = end;
    if (end == 32) {
      flush_word(w);
      w.fill = 0;
    }
  } else {
    const int over = end - 32;
    w.cur |= code >> over;
    flush_word(w);
    w.cur = code << (32 - over);
    w.fill = over;
  }
}

__global__ void __launch_bounds__(kEncThreads) jpeg_enc_emit_kernel(EncParams p) {
  const int b = (int)(blockIdx.x * kEncThreads + threadIdx.x), f = (int)blockIdx.y;
  if (b >= p.nb || p.fstate[f]) return;
  const pr_jpeg_enc_plan& plan = *p.a.plan;
  const int mcu = b / p.bpm, k = b - mcu * p.bpm;
  const int s = mcu / p.ri;
  const int t = k < p.nl ? 0 : 1;
  const long fb = (long)f * p.nb + b;
  const int pos = p.info[fb];
  BitWriter w;
  w.words = p.bits + (long)f * p.U * kChunkWords + (long)p.seg_chunk[(long)f * (p.nseg + 1) + s] * kChunkWords;
  w.word = pos >> 5;
  w.fill = pos & 31;
  w.cur = 0u;
  w.first = true;
  const int dd = p.diff[fb];
  int n = bit_length(dd < 0 ? -dd : dd);
  put_bits(w, plan.dc_code[t][n], plan.dc_len[t][n]);
  if (n) put_bits(w, (unsigned)(dd < 0 ? dd - 1 : dd) & ((1u << n) - 1u), n);
  const short* zz = p.coef + fb * 64;
  int run = 0;
  for (int z = 1; z < 64; ++z) {
    const int v = zz[z];
    if (v == 0) {
      ++run;
      continue;
    }
    for (; run > 15; run -= 16) put_bits(w, plan.ac_code[t][0xF0], plan.ac_len[t][0xF0]);
    n = bit_length(v < 0 ? -v : v);
    const int sym = run << 4 | n;
    put_bits(w, plan.ac_code[t][sym], plan.ac_len[t][sym]);
    put_bits(w, (unsigned)(v < 0 ? v - 1 : v) & ((1u << n) - 1u), n);
    run = 0;
  }
  if (run) put_bits(w, plan.ac_code[t][0], plan.ac_len[t][0]);
  const int m1 = min((s + 1) * p.ri, p.nmcu);
  if (b + 1 == m1 * p.bpm && (w.fill & 7)) {   // the segment's last block: fill its last byte with 1-bits
    const int pad = 8 - (w.fill & 7);
    put_bits(w, (1u << pad) - 1u, pad);
  }
  if (w.fill) atomicOr((int*)(w.words + w.word), (int)w.cur);
}

// ---- count, prefix, size, place -----------------------------------------------------------------------------------------------
// The segment that chunk c of frame f belongs to: the last s with seg_chunk[s] <= c (c < seg_chunk[nseg]).
__device__ __forceinline__ int segment_of(const int* seg_chunk, int nseg, int c) {
  int lo = 0, hi = nseg - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (seg_chunk[mid] <= c) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

__global__ void __launch_bounds__(kEncThreads) jpeg_enc_count_kernel(EncParams p) {
  const int c = (int)(blockIdx.x * kEncThreads + threadIdx.x), f = (int)blockIdx.y;
  if (c >= p.U || p.fstate[f]) return;
  const int* seg_chunk = p.seg_chunk + (long)f * (p.nseg + 1);
  if (c >= seg_chunk[p.nseg]) return;
  const int s = segment_of(seg_chunk, p.nseg, c);
  const int seg_bytes = (p.seg_bits[(long)f * p.nseg + s] + 7) >> 3;
  const int nvalid = min(kChunk, seg_bytes - (c - seg_chunk[s]) * kChunk);
  const unsigned* words = p.bits + ((long)f * p.U + c) * kChunkWords;
  int count = 0;
  for (int i = 0; i < nvalid; ++i) count += ((words[i >> 2] >> (24 - 8 * (i & 3))) & 255u) == 255u;
  p.ff[(long)f * p.U + c] = count;
}

__global__ void __launch_bounds__(kEncThreads) jpeg_enc_prefix_kernel(EncParams p) {
  const long i = (long)blockIdx.x * kEncThreads + threadIdx.x;
  if (i >= (long)p.a.F * p.nseg) return;
  const int f = (int)(i / p.nseg), s = (int)(i - (long)f * p.nseg);
  if (p.fstate[f]) return;
  const int* seg_chunk = p.seg_chunk + (long)f * (p.nseg + 1);
  int* ff = p.ff + (long)f * p.U;
  int total = 0;
  for (int c = seg_chunk[s]; c < seg_chunk[s + 1]; ++c) {
    const int here = ff[c];
    ff[c] = total;
    total += here;
  }
  p.seg_out[i] = ((p.seg_bits[i] + 7) >> 3) + total + 2;   // + RSTn, or EOI behind the last one
}

__global__ void __launch_bounds__(kEncThreads) jpeg_enc_size_kernel(EncParams p) {
  const int f = (int)(blockIdx.x * kEncThreads + threadIdx.x);
  if (f >= p.a.F || p.fstate[f]) return;
  int* seg_out = p.seg_out + (long)f * p.nseg;
  long off = p.a.plan->header_bytes;
  for (int s = 0; s < p.nseg; ++s) {
    const int size = seg_out[s];
    seg_out[s] = (int)min(off, 0x7fffffffl);
    off += size;
  }
  if (off > p.a.capacity) {
    p.fstate[f] = 1;
    p.a.status[f] = (int)PR_JPEG_ENC_ST_OVERFLOW;
  } else {
    p.a.nbytes[f] = (int)off;
  }
}

__global__ void __launch_bounds__(kEncThreads) jpeg_enc_place_kernel(EncParams p) {
  const int j = (int)(blockIdx.x * kEncThreads + threadIdx.x), f = (int)blockIdx.y;
  if (j >= p.U + kHeaderLanes || p.fstate[f]) return;
  unsigned char* out = p.a.out + (long)f * p.a.capacity;
  if (j < kHeaderLanes) {
    const pr_jpeg_enc_plan& plan = *p.a.plan;
    const int end = min((j + 1) * kChunk, min(plan.header_bytes, (int)PR_JPEG_ENC_HEADER_MAX));
    for (int i = j * kChunk; i < end; ++i) out[i] = plan.header[i];
    return;
  }
  const int c = j - kHeaderLanes;
  const int* seg_chunk = p.seg_chunk + (long)f * (p.nseg + 1);
  if (c >= seg_chunk[p.nseg]) return;
  const int s = segment_of(seg_chunk, p.nseg, c);
  const int seg_bytes = (p.seg_bits[(long)f * p.nseg + s] + 7) >> 3;
  const int local = (c - seg_chunk[s]) * kChunk;
  const int nvalid = min(kChunk, seg_bytes - local);
  const unsigned* words = p.bits + ((long)f * p.U + c) * kChunkWords;
  unsigned char* dst = out + p.seg_out[(long)f * p.nseg + s] + local + p.ff[(long)f * p.U + c];
  for (int i = 0; i < nvalid; ++i) {
    const unsigned byte = (words[i >> 2] >> (24 - 8 * (i & 3))) & 255u;
    *dst++ = (unsigned char)byte;
    if (byte == 255u) *dst++ = 0;
  }
  if (local + nvalid == seg_bytes) {   // the segment's last chunk
    *dst++ = 255;
    *dst++ = (unsigned char)(s + 1 < p.nseg ? 0xD0 + (s & 7) : 0xD9);
  }
}

// The workspace's arrays, one behind the other (every offset a multiple of 16 bytes).
struct EncLayout {
  size_t bits, coef, info, seg_bits, seg_chunk, seg_out, ff, fstate, diff, total;
};

// false for parameters the encoder does not accept
bool enc_geometry(int F, int H, int W, int hs, int vs, int restart_interval, int64_t capacity, EncParams* p, EncLayout* l) {
  const size_t bound = pr_jpeg_encode_bound(H, W, hs, vs, restart_interval);
  if (bound == 0 || F <= 0 || F > 65535 || capacity < 0 || capacity > 0x7fffffffl) return false;
  p->mx = (W + 8 * hs - 1) / (8 * hs);
  p->my = (H + 8 * vs - 1) / (8 * vs);
  p->nl = hs * vs;
  p->bpm = p->nl + 2;
  p->nmcu = p->mx * p->my;
  p->nb = p->nmcu * p->bpm;
  const int ri = restart_interval < 0 ? p->mx : std::min(restart_interval, 65535);
  p->ri = ri ? std::min(ri, p->nmcu) : p->nmcu;
  p->nseg = ceil_div(p->nmcu, p->ri);
  p->rbw = (W + 7) / 8;
  p->rbh = (H + 7) / 8;
  // A frame that fits has at most `capacity` bytes of unstuffed data, and rounding every segment up to whole chunks adds less
  // than one chunk a segment; more than the bound no frame has.
  p->U = (int)(std::min((size_t)capacity, bound) / kChunk) + p->nseg + 1;
  auto up = [](size_t n) { return (n + 15) & ~(size_t)15; };
  const size_t f = (size_t)F;
  size_t o = 0;
  l->bits = o, o += up(f * p->U * kChunk);
  l->coef = o, o += up(f * p->nb * 128);
  l->info = o, o += up(f * p->nb * 4);
  l->seg_bits = o, o += up(f * p->nseg * 4);
  l->seg_chunk = o, o += up(f * (p->nseg + 1) * 4);
  l->seg_out = o, o += up(f * p->nseg * 4);
  l->ff = o, o += up(f * p->U * 4);
  l->fstate = o, o += up(f * 4);
  l->diff = o, o += up(f * p->nb * 2);
  l->total = o;
  return true;
}

}  // namespace
}  // namespace pr

extern "C" size_t pr_jpeg_encode_workspace_bytes(int F, int H, int W, int hs, int vs, int restart_interval, int64_t capacity) {
  pr::EncParams p;
  pr::EncLayout l;
  return pr::enc_geometry(F, H, W, hs, vs, restart_interval, capacity, &p, &l) ? l.total : 0;
}

extern "C" int pr_jpeg_encode(const pr_jpeg_enc_args* a, void* workspace, size_t workspace_bytes, void* stream) {
  using namespace pr;
  PR_REQUIRE(a, "pr_jpeg_encode: null argument struct");
  PR_REQUIRE(a->F >= 0, "pr_jpeg_encode: F = %d", a->F);
  if (a->F == 0) return PR_OK;
  EncParams p;
  EncLayout l;
  PR_REQUIRE(enc_geometry(a->F, a->H, a->W, a->hs, a->vs, a->restart_interval, a->capacity, &p, &l),
             "pr_jpeg_encode: %d frames of %d x %d, sampling %d x %d, restart interval %d, capacity %lld: at most 65535 frames, "
             "sizes 16..4096, sampling 1x1, 2x1 or 2x2, the interval -1, 0 or a count of MCUs, capacity 0..2^31-1",
             a->F, a->W, a->H, a->hs, a->vs, a->restart_interval, (long long)a->capacity);
  PR_REQUIRE(a->frames, "pr_jpeg_encode: null frames");
  PR_REQUIRE(a->plan, "pr_jpeg_encode: null plan");
  PR_REQUIRE(a->out || a->capacity == 0, "pr_jpeg_encode: null out");
  PR_REQUIRE(a->nbytes, "pr_jpeg_encode: null nbytes");
  PR_REQUIRE(a->status, "pr_jpeg_encode: null status");
  PR_REQUIRE(workspace, "pr_jpeg_encode: null workspace");
  PR_REQUIRE(((uintptr_t)workspace & 15) == 0, "pr_jpeg_encode: workspace is not 16-byte aligned");
  PR_REQUIRE(workspace_bytes >= l.total, "pr_jpeg_encode: workspace of %zu bytes, %zu needed for %d frames of %d x %d",
             workspace_bytes, l.total, a->F, a->H, a->W);
  p.a = *a;
  char* ws = (char*)workspace;
  p.bits = (unsigned*)(ws + l.bits);
  p.coef = (short*)(ws + l.coef);
  p.info = (int*)(ws + l.info);
  p.seg_bits = (int*)(ws + l.seg_bits);
  p.seg_chunk = (int*)(ws + l.seg_chunk);
  p.seg_out = (int*)(ws + l.seg_out);
  p.ff = (int*)(ws + l.ff);
  p.fstate = (int*)(ws + l.fstate);
  p.diff = (short*)(ws + l.diff);
  hipStream_t s = (hipStream_t)stream;
  const unsigned F = (unsigned)a->F;
  const dim3 threads(kEncThreads);
  const dim3 per_block((unsigned)ceil_div(p.nb, kEncThreads), F), per_segment((unsigned)ceil_div((long)a->F * p.nseg, (long)kEncThreads)),
      per_frame((unsigned)ceil_div(a->F, kEncThreads)), per_chunk((unsigned)ceil_div(p.U + kHeaderLanes, kEncThreads), F);
  PR_HIP(hipMemsetAsync(p.bits, 0, (size_t)a->F * p.U * kChunk, s));
  hipLaunchKernelGGL(jpeg_enc_transform_kernel, per_block, threads, 0, s, p);
  PR_TRY(check_launch("jpeg_enc_transform_kernel"));
  hipLaunchKernelGGL(jpeg_enc_scan_kernel, per_segment, threads, 0, s, p);
  PR_TRY(check_launch("jpeg_enc_scan_kernel"));
  hipLaunchKernelGGL(jpeg_enc_layout_kernel, per_frame, threads, 0, s, p);
  PR_TRY(check_launch("jpeg_enc_layout_kernel"));
  hipLaunchKernelGGL(jpeg_enc_emit_kernel, per_block, threads, 0, s, p);
  PR_TRY(check_launch("jpeg_enc_emit_kernel"));
  hipLaunchKernelGGL(jpeg_enc_count_kernel, per_chunk, threads, 0, s, p);
  PR_TRY(check_launch("jpeg_enc_count_kernel"));
  hipLaunchKernelGGL(jpeg_enc_prefix_kernel, per_segment, threads, 0, s, p);
  PR_TRY(check_launch("jpeg_enc_prefix_kernel"));
  hipLaunchKernelGGL(jpeg_enc_size_kernel, per_frame, threads, 0, s, p);
  PR_TRY(check_launch("jpeg_enc_size_kernel"));
  hipLaunchKernelGGL(jpeg_enc_place_kernel, per_chunk, threads, 0, s, p);
  return check_launch("jpeg_enc_place_kernel");
}
