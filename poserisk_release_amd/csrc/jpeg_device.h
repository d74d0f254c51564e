// What csrc/jpeg.hip (one lane per restart segment) and csrc/jpeg_sync.hip (one lane per sub-sequence) share: the kernels' argument
// block, a frame's geometry, the descriptor check and the bit reader with Huffman decode.  Included after common.h (or the
// host shim that stands in for it in the CPU tests): this file includes nothing itself.
#pragma once

namespace pr {
// The kernels' argument block (outside the unnamed namespace: the two launchers at this file's end take it across files).
struct JpegParams {
  pr_jpeg_args a;
  short* coef;             // [F][cs] int16, natural order inside a block, blocks row-major per component
  unsigned char* planes;   // [F][cs] u8, component planes at block-padded size
  long cs;                 // samples per frame in either: 3 * roundup(W, 16) * roundup(H, 16)
  int out_aligned;         // out is 4-byte aligned: the colour kernel stores dwords
  int lanes;               // segments per wave of the entropy kernel, 1..64
  const pr_jpeg_sync_stats* gate;   // null, or [F]: the serial entropy kernel decodes only frames with gate[f].fell_back set
};

namespace {

static __device__ const unsigned char kZigzagNatural[64] = {
    0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28,
    35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// Where a frame's components live inside its cs samples; the same offsets serve coefficients and planes.
struct Geometry {
  int mx, my;          // MCUs across and down
  int bw[3], bh[3];    // blocks across and down per component
  long off[3];         // first sample per component
};

// Every descriptor field that later forms an address or a loop bound.  A frame that fails is never decoded: its pixels are zero
// and its status PR_JPEG_ST_REFUSED.
__device__ __forceinline__ bool frame_ok(const pr_jpeg_frame& f, const pr_jpeg_args& a) {
  if (f.width != a.W || f.height != a.H) return false;
  if (f.ncomp != 1 && f.ncomp != 3) return false;
  const bool s11 = f.hs == 1 && f.vs == 1, s21 = f.hs == 2 && f.vs == 1, s22 = f.hs == 2 && f.vs == 2;
  if (!(s11 || (f.ncomp == 3 && (s21 || s22)))) return false;
  if ((unsigned)f.huff_set >= (unsigned)a.n_huff || f.restart_interval < 0) return false;
  for (int c = 0; c < 3; ++c)
    if ((unsigned)f.dc_sel[c] > 1u || (unsigned)f.ac_sel[c] > 1u) return false;
  return true;
}

__device__ __forceinline__ Geometry geometry(const pr_jpeg_frame& f) {   // of a frame that passed frame_ok
  Geometry g;
  g.mx = (f.width + 8 * f.hs - 1) / (8 * f.hs);
  g.my = (f.height + 8 * f.vs - 1) / (8 * f.vs);
  g.bw[0] = g.mx * f.hs;
  g.bh[0] = g.my * f.vs;
  g.bw[1] = g.bw[2] = g.mx;
  g.bh[1] = g.bh[2] = g.my;
  g.off[0] = 0;
  g.off[1] = (long)g.bw[0] * g.bh[0] * 64;
  g.off[2] = g.off[1] + (long)g.mx * g.my * 64;   // <= 3 roundup(W,16) roundup(H,16) - mx my 64 for every accepted sampling
  return g;
}

// ---- entropy decoding -----------------------------------------------------------------------------------------------------
// The bit reader of one segment.  acc holds cnt valid bits in its low end; `pad` of them (the lowest) are zeros made up
// because the data ended: consuming one of those sets PR_JPEG_ST_TRUNCATED.  pos never leaves [begin, end].  A refill takes four
// bytes with one load where none of them is 0xFF (the common case: an encoder's output is close to uniform bytes) and goes
// byte by byte, unstuffing, otherwise and at the segment's end.  With Track (csrc/jpeg_sync.hip) `marks` holds one bit per
// buffered byte, youngest lowest: set where a stuffed 00 was skipped behind that byte, which is what bit_position needs.
struct Bits {
  const unsigned char* data;
  long pos, end;
  unsigned long long acc;
  int cnt, pad;
  bool ended;
  int st;
  unsigned marks;
};

template <bool Track = false>
__device__ __forceinline__ void fill(Bits& b) {
  if (b.cnt > 24) return;
  if (!b.ended && b.pos + 4 <= b.end) {
    unsigned w;
    __builtin_memcpy(&w, b.data + b.pos, 4);                 // any alignment
    if (((~w - 0x01010101u) & w & 0x80808080u) == 0u) {      // no byte of w is 0xFF
      b.acc = (b.acc << 32) | __builtin_bswap32(w);
      b.cnt += 32;
      b.pos += 4;
      if (Track) b.marks <<= 4;
      return;
    }
  }
  while (b.cnt <= 24) {
    unsigned byte = 0u;
    if (Track) b.marks <<= 1;
    if (!b.ended && b.pos < b.end) {
      byte = b.data[b.pos];
      if (byte == 0xFFu) {
        if (b.pos + 1 < b.end && b.data[b.pos + 1] == 0u) {
          b.pos += 2;                 // a stuffed 0xFF
          if (Track) b.marks |= 1u;
        } else {
          b.ended = true;             // a marker, fill bytes or a lone 0xFF at the end: no data behind it
          byte = 0u;
        }
      } else {
        ++b.pos;
      }
    } else {
      b.ended = true;
    }
    if (b.ended) b.pad += 8;
    b.acc = (b.acc << 8) | byte;
    b.cnt += 8;
  }
}

__device__ __forceinline__ unsigned peek(const Bits& b, int n) {   // 1 <= n <= 16 <= cnt
  return (unsigned)(b.acc >> (b.cnt - n)) & ((1u << n) - 1u);
}

__device__ __forceinline__ void consume(Bits& b, int n) {
  b.cnt -= n;
  if (b.cnt < b.pad) {
    b.st |= PR_JPEG_ST_TRUNCATED;
    b.pad = b.cnt;
  }
}

// The next Huffman symbol, or -1 when no code of the table matches.
template <bool Track = false>
__device__ __forceinline__ int next_symbol(Bits& b, const pr_jpeg_hufftab& t) {
  fill<Track>(b);
  const unsigned e = t.look[peek(b, PR_JPEG_LOOK_BITS)];
  if (e) {
    consume(b, (int)(e >> 8) & 15);
    return (int)(e & 255u);
  }
  for (int l = PR_JPEG_LOOK_BITS + 1; l <= 16; ++l) {
    const int code = (int)peek(b, l);
    if (code <= t.maxcode[l]) {
      consume(b, l);
      return t.vals[(t.valoff[l] + code) & 255];
    }
  }
  return -1;
}

template <bool Track = false>
__device__ __forceinline__ int receive_extend(Bits& b, int s) {   // 1 <= s <= 15
  fill<Track>(b);
  const int r = (int)peek(b, s);
  consume(b, s);
  return r < (1 << (s - 1)) ? r - (1 << s) + 1 : r;
}

inline long padded_samples(int H, int W) { return 3l * ((W + 15) & ~15) * ((H + 15) & ~15); }

}  // namespace

// The back half of every decode (csrc/jpeg.hip): the serial entropy kernel, for the frames whose gate[f].fell_back is set when
// p.gate is given and for every frame otherwise, and dequantise + IDCT + colour over all frames.
int jpeg_launch_serial_entropy(const JpegParams& p, hipStream_t s);
int jpeg_launch_back_end(const JpegParams& p, hipStream_t s);
}  // namespace pr
