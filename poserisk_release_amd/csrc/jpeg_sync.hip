// Entropy decoding of a JPEG scan by self-synchronising sub-sequences: the front of pr_jpeg_decode_sync.  The contract is in
// include/poserisk_hip.h (section j1); the method and its measurements are in DESIGN.md section 3.9.
//
// Two baseline Huffman decoders on one scan share their future once they agree on (next unread bit, block slot of the MCU,
// next zig-zag index).  Every restart segment is cut into sub-sequences of S raw bytes, ONE LANE each:
//   map      one lane per segment: checks the segment as the serial kernel does and deals it its lanes.  Segment i owns lanes
//            begin / S + i ... + ceil(length / S) - 1: disjoint for the parser's segments (ascending, not overlapping), inside
//            data_bytes / S + n_segments + 1 for any, and computable without a scan over the segments.
//   cold     lane s decodes its sub-sequence from (first bit, slot 0, index 0) -- true for lane 0 of a segment, a guess for
//            the others -- up to the first symbol boundary at or behind the sub-sequence's end, and keeps the exit state, the
//            number of blocks begun and completed and the sum of the DC differences per component.  Nothing else is written.
//   round j  (one launch each, states ping-ponged: a Jacobi iteration) lane s decodes again from lane s - 1's exit of the
//            round before, unless that is the entry it used last; an exit that differs from the round before marks the frame
//            as changed in round j.  A frame is converged at the first round that changes nothing: by induction from lane 0
//            every entry state is then the serial decoder's.  Later rounds return at once for it.  Round 1 counts every lane
//            s >= 2 as changed: its entry came from a guess's exit.  A lane whose entry is DEAD (the lane in front met a code
//            no table holds or ran out of data -- guesses do that all the time) decodes from its own guess again, so that
//            the lanes behind it can still synchronise; a run past coefficient 63 ends the block, as in the serial kernel.
//   scan     one lane per segment: the converged round into the statistics, exclusive prefix sums of blocks begun (the block
//            ordinal a sub-sequence starts at) and of the DC sums (the prediction it starts from); a segment that completes
//            fewer blocks than it holds raises PR_JPEG_ST_TRUNCATED; every lane behind the first DEAD exit of the converged
//            states is marked, and the write pass skips it.  A frame that did not converge in R rounds, or whose
//            lanes another segment claimed (descriptors no parser wrote), is marked fell_back.
//   write    lane s decodes once more from its converged entry, scatters the non-zero coefficients to the serial kernel's
//            addresses (ordinal -> MCU, slot -> Geometry) with the final DC values, and stops at the segment's block count;
//            status bits are raised here and in scan only, and only for blocks below that count.
// Frames marked fell_back are then decoded by the serial kernel of csrc/jpeg.hip (on the device: it reads the mark), and the
// IDCT and colour kernels run as for pr_jpeg_decode.  The DC prediction needs no pass of its own: the sums ride along with the
// block counts.  Kernels index by thread only: no LDS, no barrier, no cross-lane operation, so tests/test_jpeg_sync_native.py
// runs this file on the host under sanitizers exactly as tests/test_jpeg_native.py runs jpeg.hip.
#include "common.h"
#include "jpeg_device.h"

#ifndef PR_JPEG_SYNC_SUBSEQ_BYTES
#define PR_JPEG_SYNC_SUBSEQ_BYTES 128
#endif
#ifndef PR_JPEG_SYNC_MAX_ROUNDS
#define PR_JPEG_SYNC_MAX_ROUNDS 16
#endif
// Lanes are dealt to waves as the serial kernel's are: the fewest lanes a wave that still fit every sub-sequence into this
// many waves a CU (a data-dependent branch is paid once per path taken in a wave).  DESIGN.md section 3.9 has what was measured.
#ifndef PR_JPEG_SYNC_WAVES_PER_CU
#define PR_JPEG_SYNC_WAVES_PER_CU 16
#endif

namespace pr {
namespace {

constexpr int kSyncThreads = 64;
constexpr unsigned long long kDead = ~0ull;   // a state: (bit position relative to the segment << 10) | slot << 6 | index

struct SyncParams {
  JpegParams j;
  pr_jpeg_sync_stats* stats;        // [F]; fell_back doubles as the serial kernel's gate
  unsigned long long* state[2];     // [T] exit states, ping-ponged
  unsigned long long* used;         // [T] the entry state a lane's kept results belong to
  unsigned* counts;                 // [T] blocks begun << 16 | blocks completed
  int* dcsum;                       // [T][3] sum of DC differences per component
  int* start;                       // [T] ordinal of the first block begun in the sub-sequence
  int* dcbase;                      // [T][3] DC prediction in front of the sub-sequence
  int* owner;                       // [T] segment a lane works for, -1 = none
  int* changed;                     // [F][R + 1]
  long T;
  int S, R, round, lanes;
};

// A segment that may be decoded: the serial kernel's checks, in its order.
struct SegInfo {
  pr_jpeg_segment sg;
  long base;       // first lane
  int n;           // sub-sequences = lanes
  int count;       // blocks the segment holds
  int bpm, hv;     // blocks per MCU, luma blocks per MCU
};

__device__ __forceinline__ bool segment_info(const SyncParams& p, int i, SegInfo& o, bool report) {
  const pr_jpeg_args& a = p.j.a;
  o.sg = a.segments[i];
  if ((unsigned)o.sg.frame >= (unsigned)a.F) return false;
  const pr_jpeg_frame& fr = a.frames[o.sg.frame];
  if (!frame_ok(fr, a)) return false;
  const int total = ((fr.width + 8 * fr.hs - 1) / (8 * fr.hs)) * ((fr.height + 8 * fr.vs - 1) / (8 * fr.vs));
  if (o.sg.begin < 0 || o.sg.end > a.data_bytes || o.sg.begin > o.sg.end || o.sg.first_mcu < 0 || o.sg.first_mcu >= total) {
    if (report) atomicOr(a.status + o.sg.frame, (int)PR_JPEG_ST_REFUSED);
    return false;
  }
  const int n_mcus = fr.restart_interval > 0 ? min(fr.restart_interval, total - o.sg.first_mcu) : total - o.sg.first_mcu;
  o.hv = fr.ncomp == 1 ? 1 : fr.hs * fr.vs;
  o.bpm = fr.ncomp == 1 ? 1 : o.hv + 2;
  o.count = n_mcus * o.bpm;                                    // <= 6 * 512 * 512
  o.base = o.sg.begin / p.S + i;
  o.n = (int)((o.sg.end - o.sg.begin + p.S - 1) / p.S);       // data_bytes / 16 < 2^31 is checked by the entry point
  return o.base + o.n <= p.T;
}

__global__ void __launch_bounds__(kSyncThreads) jpeg_sync_map_kernel(SyncParams p) {
  const int i = (int)blockIdx.x * kSyncThreads + (int)threadIdx.x;
  if (i >= p.j.a.n_segments) return;
  SegInfo si;
  if (!segment_info(p, i, si, true)) return;
  for (int s = 0; s < si.n; ++s) p.owner[si.base + s] = i;
  if (si.n) atomicAdd(&p.stats[si.sg.frame].n_subseq, si.n);
}

// The raw position of the next unread bit: never inside a stuffed 00 (a 00 skipped behind a byte that is still buffered, wholly
// or in part, lies ahead).
__device__ __forceinline__ long bit_position(const Bits& b) {
  const unsigned buffered = (1u << ((b.cnt + 7) >> 3)) - 1u;   // cnt <= 56
  return b.pos * 8 - (b.cnt - b.pad) - 8 * __builtin_popcount(b.marks & buffered);
}

struct Lane {
  const unsigned char* data;
  long begin, end;                 // the segment
  const pr_jpeg_hufftab* tab;      // the frame's four tables; bit c of dc_sel / ac_sel picks component c's (no indexed arrays:
  int dc_sel, ac_sel;              // they would live in scratch memory)
  int bpm, hv;
  // the write pass only
  short* coef;
  int* status;
  Geometry g;
  int hs, vs, first_mcu, count;
};

__device__ __forceinline__ short* block_address(const Lane& L, int ordinal) {   // 0 <= ordinal < L.count
  const int m = ordinal / L.bpm, slot = ordinal - m * L.bpm, mcu = L.first_mcu + m;
  const int mxi = mcu % L.g.mx, myi = mcu / L.g.mx;
  const int c = slot < L.hv ? 0 : slot - L.hv + 1, blk = c == 0 ? slot : 0;
  const int hc = c == 0 ? L.hs : 1, vc = c == 0 ? L.vs : 1;
  const int bx = mxi * hc + blk % hc, by = myi * vc + blk / hc;
  const long off = c == 0 ? 0l : (c == 1 ? L.g.off[1] : L.g.off[2]);
  return L.coef + off + ((long)by * (c == 0 ? L.g.bw[0] : L.g.mx) + bx) * 64;
}

// One sub-sequence from `entry` to the first symbol boundary at or behind `limit` (bits from the segment's begin) -> the exit
// state.  A symbol that consumes a made-up bit behind the data's end is not taken: the lane ends DEAD in front of it.  Write:
// `ordinal` is the first block begun here (a block continued from the lane before is ordinal - 1), `dc` the predictions in
// front of it; blocks at or past L.count are neither written nor reported.
template <bool Write>
__device__ __forceinline__ unsigned long long decode_subseq(const Lane& L, unsigned long long entry, long limit, int& begun, int& done,
                                                            int& dc0, int& dc1, int& dc2, int ordinal) {
  begun = done = 0;
  if (entry == kDead) return kDead;
  const long p0 = (long)(entry >> 10);
  int u = (int)(entry >> 6) & 15, k = (int)entry & 63;
  if (u >= L.bpm || p0 > (L.end - L.begin) * 8) return kDead;
  Bits b;
  b.data = L.data;
  b.pos = L.begin + (p0 >> 3);
  b.end = L.end;
  b.acc = 0ull;
  b.cnt = 0;
  b.pad = 0;
  b.ended = false;
  b.st = 0;
  b.marks = 0u;
  if (p0 & 7) {
    fill<true>(b);
    consume(b, (int)(p0 & 7));
    if (b.st) return kDead;
  }
  short* out = nullptr;
  if (Write && k > 0) {
    if (ordinal < 1) return kDead;
    if (ordinal - 1 < L.count) out = block_address(L, ordinal - 1);
  }
  int bad = 0;
  for (;;) {
    long here = b.pos * 8 - (b.cnt - b.pad);                     // an upper bound unless stuffed bytes are buffered
    if (here - L.begin * 8 >= limit) {
      here = bit_position(b);
      if (here - L.begin * 8 >= limit) return (unsigned long long)(here - L.begin * 8) << 10 | (unsigned)(u << 6 | k);
    }
    if (Write && ordinal - (k > 0) >= L.count) return kDead;     // the segment's blocks are done: what follows is not data
    const int c = u < L.hv ? 0 : u - L.hv + 1;
    if (k == 0) {
      const int s = next_symbol<true>(b, L.tab[(L.dc_sel >> c) & 1]);
      if (s < 0 || s > 15) {
        bad = PR_JPEG_ST_BAD_CODE;
        break;
      }
      const int diff = s ? receive_extend<true>(b, s) : 0;
      if (b.st) break;
      ++begun;
      dc0 += c == 0 ? diff : 0;
      dc1 += c == 1 ? diff : 0;
      dc2 += c == 2 ? diff : 0;
      if (Write) {
        out = block_address(L, ordinal);
        ++ordinal;
        int v = c == 0 ? dc0 : (c == 1 ? dc1 : dc2);
        if (v != (short)v) {
          atomicOr(L.status, (int)PR_JPEG_ST_COEF_RANGE);
          v = v < 0 ? -32768 : 32767;
        }
        if (v) out[0] = (short)v;
      }
      k = 1;
      continue;
    }
    const int rs = next_symbol<true>(b, L.tab[2 + ((L.ac_sel >> c) & 1)]);
    if (rs < 0) {
      bad = PR_JPEG_ST_BAD_CODE;
      break;
    }
    const int r = rs >> 4, s = rs & 15;
    bool ends = false, overrun = false;
    if (s == 0) {
      if (b.st) break;
      if (r == 15) {
        k += 16;
        if (k <= 63) continue;
        overrun = true;
      } else {
        ends = true;                                             // end of block
      }
    } else {
      k += r;
      if (k <= 63) {
        const int v = receive_extend<true>(b, s);
        if (b.st) break;
        if (Write) out[kZigzagNatural[k]] = (short)v;
        ends = ++k == 64;
      } else {
        overrun = true;
      }
    }
    if (overrun) {                                               // a run past 63 ends the block, as in the serial kernel
      if (Write) atomicOr(L.status, (int)PR_JPEG_ST_BAD_RUN);
      ends = true;
    }
    if (ends) {
      ++done;
      k = 0;
      u = u + 1 == L.bpm ? 0 : u + 1;
    }
  }
  // DEAD: a code no table holds, or the data ended inside a symbol (the scan kernel reports the missing blocks)
  if (Write && bad && ordinal - (k > 0) < L.count) atomicOr(L.status, bad);
  return kDead;
}

// round 0 = cold, 1 .. R = the iteration, R + 1 = the write pass
__global__ void __launch_bounds__(kSyncThreads) jpeg_sync_decode_kernel(SyncParams p) {
  const long t = (long)blockIdx.x * p.lanes + (long)threadIdx.x;
  if ((int)threadIdx.x >= p.lanes || t >= p.T) return;
  const int i = p.owner[t];
  if ((unsigned)i >= (unsigned)p.j.a.n_segments) return;
  {  // a converged frame's lanes leave before anything else is loaded or divided
    const int frame = p.j.a.segments[i].frame, r = p.round;
    if ((unsigned)frame >= (unsigned)p.j.a.F) return;
    if (r >= 2 && r <= p.R && p.changed[(long)frame * (p.R + 1) + r - 1] == 0) return;
  }
  SegInfo si;
  if (!segment_info(p, i, si, false)) return;
  const long s = t - si.base;
  if (s < 0 || s >= si.n) return;
  const pr_jpeg_args& a = p.j.a;
  const int f = si.sg.frame, j = p.round;
  const bool writing = j == p.R + 1;
  int* changed = p.changed + (long)f * (p.R + 1);
  if (writing ? p.stats[f].fell_back != 0 : (j >= 2 && changed[j - 1] == 0)) return;
  const unsigned long long* from = p.state[(j + 1) & 1];          // the round before (the write pass: either, they are equal)
  unsigned long long* to = p.state[j & 1];
  const long c0 = si.sg.begin + s * p.S, c1 = min(c0 + p.S, si.sg.end);
  const bool inside_pair = s > 0 && a.data[c0] == 0u && a.data[c0 - 1] == 0xFFu;     // c0 - 1 >= begin, c0 < end
  const unsigned long long guess = (unsigned long long)((c0 - si.sg.begin + (inside_pair ? 1 : 0)) * 8) << 10;
  const unsigned long long given = s == 0 || j == 0 ? guess : from[t - 1];
  unsigned long long entry = given;
  if (j >= 1 && !writing) {
    const bool unproven = j == 1 && s >= 2;
    if (s == 0 || given == p.used[t]) {
      to[t] = from[t];
      if (unproven) atomicOr(changed + j, 1);
      return;
    }
    // A dead lane in front says nothing about where this one's symbols lie: it keeps its guess, so that the lanes behind it
    // can still synchronise.  Whether the segment really died is the scan kernel's to say, from the converged states.
    if (entry == kDead) entry = guess;
  }
  const pr_jpeg_frame& fr = a.frames[f];
  const pr_jpeg_huff& tabs = a.huff[fr.huff_set];
  Lane L;
  L.data = a.data;
  L.begin = si.sg.begin;
  L.end = si.sg.end;
  L.tab = tabs.tab;
  L.dc_sel = fr.dc_sel[0] | fr.dc_sel[1] << 1 | fr.dc_sel[2] << 2;   // each 0 or 1: frame_ok
  L.ac_sel = fr.ac_sel[0] | fr.ac_sel[1] << 1 | fr.ac_sel[2] << 2;
  L.bpm = si.bpm;
  L.hv = si.hv;
  L.coef = p.j.coef + (long)f * p.j.cs;
  L.status = a.status + f;
  L.g = geometry(fr);
  L.hs = fr.hs;
  L.vs = fr.vs;
  L.first_mcu = si.sg.first_mcu;
  L.count = si.count;
  const long limit = (c1 - si.sg.begin) * 8;
  int begun, done;
  if (writing) {
    if (p.start[t] < 0) return;                                   // behind the lane in which the segment died
    int dc0 = p.dcbase[3 * t], dc1 = p.dcbase[3 * t + 1], dc2 = p.dcbase[3 * t + 2];
    decode_subseq<true>(L, entry, limit, begun, done, dc0, dc1, dc2, p.start[t]);
    return;
  }
  int dc0 = 0, dc1 = 0, dc2 = 0;
  const unsigned long long left = decode_subseq<false>(L, entry, limit, begun, done, dc0, dc1, dc2, 0);
  p.used[t] = given;
  to[t] = left;
  p.counts[t] = (unsigned)begun << 16 | (unsigned)done;           // at most one block per two bits of 4096 + 4 bytes
  p.dcsum[3 * t] = dc0;
  p.dcsum[3 * t + 1] = dc1;
  p.dcsum[3 * t + 2] = dc2;
  if (j >= 1 && (left != from[t] || (j == 1 && s >= 2))) atomicOr(changed + j, 1);
}

__global__ void __launch_bounds__(kSyncThreads) jpeg_sync_scan_kernel(SyncParams p) {
  const int i = (int)blockIdx.x * kSyncThreads + (int)threadIdx.x;
  if (i >= p.j.a.n_segments) return;
  SegInfo si;
  if (!segment_info(p, i, si, false)) return;
  const int f = si.sg.frame;
  const int* changed = p.changed + (long)f * (p.R + 1);
  int rounds = 0;
  for (int j = 1; j <= p.R && !rounds; ++j)
    if (changed[j] == 0) rounds = j;
  atomicMax(&p.stats[f].rounds, rounds ? rounds : p.R);           // every segment of the frame has the same value, unless ...
  if (!rounds) {
    atomicOr(&p.stats[f].fell_back, 1);
    return;
  }
  int ordinal = 0, done = 0, dc[3] = {0, 0, 0};
  bool died = false;
  for (int s = 0; s < si.n; ++s) {
    const long t = si.base + s;
    if (p.owner[t] != i) {                                        // overlapping segments: no parser writes those
      atomicOr(&p.stats[f].fell_back, 1);
      atomicMax(&p.stats[f].rounds, p.R);                         // ... it falls back here: rounds = R then, as documented
      return;
    }
    // hostile bytes can begin more blocks than the segment holds: lanes wholly behind its last block have nothing to write, and
    // the sums stop there, so that they stay below count + 2^16 whatever the segment's length
    if (ordinal > si.count) died = true;
    p.start[t] = died ? -1 : ordinal;
    if (died) continue;
    died = p.state[0][t] == kDead;                                // converged: both state arrays hold the same
    const unsigned n = p.counts[t];
    ordinal += (int)(n >> 16);
    done += (int)(n & 0xFFFFu);
    for (int c = 0; c < 3; ++c) {
      p.dcbase[3 * t + c] = dc[c];
      dc[c] += p.dcsum[3 * t + c];                                // |.| < 2^15 * 2^15 a lane: clamp so that no sum of lanes wraps
      dc[c] = dc[c] > (1 << 24) ? (1 << 24) : (dc[c] < -(1 << 24) ? -(1 << 24) : dc[c]);
    }
  }
  if (done < si.count) atomicOr(p.j.a.status + f, (int)PR_JPEG_ST_TRUNCATED);
}

inline size_t round16(size_t n) { return (n + 15) & ~(size_t)15; }

struct SyncLayout {
  size_t state[2], used, counts, dcsum, start, dcbase, owner, changed, stats, total;
  long T;
};

inline SyncLayout sync_layout(int F, int H, int W, int64_t data_bytes, int n_segments, int S, int R) {
  SyncLayout l;
  l.T = (long)(data_bytes / S) + n_segments + 1;
  size_t at = (size_t)F * (size_t)padded_samples(H, W) * 3u;
  auto take = [&](size_t bytes) {
    const size_t here = at;
    at += round16(bytes);
    return here;
  };
  const size_t T = (size_t)l.T;
  l.state[0] = take(T * 8);
  l.state[1] = take(T * 8);
  l.used = take(T * 8);
  l.counts = take(T * 4);
  l.dcsum = take(T * 12);
  l.start = take(T * 4);
  l.dcbase = take(T * 12);
  l.owner = take(T * 4);
  l.changed = take((size_t)F * (R + 1) * 4);
  l.stats = take((size_t)F * sizeof(pr_jpeg_sync_stats));
  l.total = at;
  return l;
}

inline bool sync_opts(const pr_jpeg_sync_opts* o, int* S, int* R) {
  *S = o && o->subseq_bytes ? o->subseq_bytes : PR_JPEG_SYNC_SUBSEQ_BYTES;
  *R = o ? o->max_rounds : PR_JPEG_SYNC_MAX_ROUNDS;           // no 0 here: a caller that names rounds names a number
  return *S >= 16 && *S <= 4096 && *S % 4 == 0 && *R >= 1 && *R <= 64;
}

}  // namespace
}  // namespace pr

extern "C" size_t pr_jpeg_sync_workspace_bytes(int F, int H, int W, int64_t data_bytes, int n_segments, const pr_jpeg_sync_opts* opts) {
  int S, R;
  if (F <= 0 || H <= 0 || W <= 0 || H > 4096 || W > 4096 || data_bytes < 0 || n_segments < 0 || !pr::sync_opts(opts, &S, &R)) return 0;
  if (data_bytes / 16 + n_segments >= (1ll << 31) - 1) return 0;
  return pr::sync_layout(F, H, W, data_bytes, n_segments, S, R).total;
}

extern "C" int pr_jpeg_decode_sync(const pr_jpeg_args* a, const pr_jpeg_sync_opts* opts, pr_jpeg_sync_stats* stats, void* workspace,
                                   size_t workspace_bytes, void* stream) {
  using namespace pr;
  PR_REQUIRE(a, "pr_jpeg_decode_sync: null argument struct");
  PR_REQUIRE(a->F >= 0, "pr_jpeg_decode_sync: F = %d", a->F);
  int S, R;
  PR_REQUIRE(sync_opts(opts, &S, &R),
             "pr_jpeg_decode_sync: subseq_bytes = %d (a multiple of 4 in 16..4096, or 0 for %d), max_rounds = %d (1..64)",
             opts ? opts->subseq_bytes : 0, PR_JPEG_SYNC_SUBSEQ_BYTES, opts ? opts->max_rounds : 0);
  if (a->F == 0) return PR_OK;
  PR_REQUIRE(a->F <= 65535, "pr_jpeg_decode_sync: F = %d frames in one call (at most 65535)", a->F);
  PR_REQUIRE(a->H >= 16 && a->W >= 16 && a->H <= 4096 && a->W <= 4096, "pr_jpeg_decode_sync: H x W = %d x %d outside 16..4096",
             a->H, a->W);
  PR_REQUIRE(a->frames, "pr_jpeg_decode_sync: null frames");
  PR_REQUIRE(a->out, "pr_jpeg_decode_sync: null out");
  PR_REQUIRE(a->status, "pr_jpeg_decode_sync: null status");
  PR_REQUIRE(a->n_segments >= 0 && a->n_huff >= 0 && a->data_bytes >= 0,
             "pr_jpeg_decode_sync: negative count (n_segments %d, n_huff %d, data_bytes %lld)", a->n_segments, a->n_huff,
             (long long)a->data_bytes);
  PR_REQUIRE(a->n_segments == 0 || (a->segments && a->data && a->huff && a->n_huff > 0 && a->data_bytes > 0),
             "pr_jpeg_decode_sync: %d segments need data, segments and huff (null pointer, n_huff = %d or data_bytes = %lld)",
             a->n_segments, a->n_huff, (long long)a->data_bytes);
  PR_REQUIRE(workspace, "pr_jpeg_decode_sync: null workspace");
  PR_REQUIRE(((uintptr_t)workspace & 15) == 0, "pr_jpeg_decode_sync: workspace is not 16-byte aligned");
  const size_t need = pr_jpeg_sync_workspace_bytes(a->F, a->H, a->W, a->data_bytes, a->n_segments, opts);
  PR_REQUIRE(need != 0, "pr_jpeg_decode_sync: %lld bytes in %d segments are too many for one call", (long long)a->data_bytes,
             a->n_segments);
  PR_REQUIRE(workspace_bytes >= need, "pr_jpeg_decode_sync: workspace of %zu bytes, %zu needed for %d frames of %d x %d",
             workspace_bytes, need, a->F, a->H, a->W);
  const long quads = ceil_div((long)a->F * a->H * a->W, 4l);
  PR_REQUIRE(quads <= (1l << 38), "pr_jpeg_decode_sync: %d frames of %d x %d are too many pixels for one call", a->F, a->H, a->W);
  const SyncLayout l = sync_layout(a->F, a->H, a->W, a->data_bytes, a->n_segments, S, R);
  unsigned char* ws = (unsigned char*)workspace;
  SyncParams p;
  p.j.a = *a;
  p.j.cs = padded_samples(a->H, a->W);
  p.j.out_aligned = ((uintptr_t)a->out & 3) == 0;
  p.j.lanes = 1;
  p.j.coef = (short*)ws;
  p.j.planes = ws + (size_t)a->F * p.j.cs * 2;
  p.stats = stats ? stats : (pr_jpeg_sync_stats*)(ws + l.stats);
  p.j.gate = p.stats;
  p.state[0] = (unsigned long long*)(ws + l.state[0]);
  p.state[1] = (unsigned long long*)(ws + l.state[1]);
  p.used = (unsigned long long*)(ws + l.used);
  p.counts = (unsigned*)(ws + l.counts);
  p.dcsum = (int*)(ws + l.dcsum);
  p.start = (int*)(ws + l.start);
  p.dcbase = (int*)(ws + l.dcbase);
  p.owner = (int*)(ws + l.owner);
  p.changed = (int*)(ws + l.changed);
  p.T = l.T;
  p.S = S;
  p.R = R;
  p.round = 0;
  p.lanes = kSyncThreads;
  hipStream_t s = (hipStream_t)stream;
  PR_HIP(hipMemsetAsync(p.j.coef, 0, (size_t)a->F * p.j.cs * 2, s));
  PR_HIP(hipMemsetAsync(a->status, 0, (size_t)a->F * sizeof(int32_t), s));
  PR_HIP(hipMemsetAsync(p.stats, 0, (size_t)a->F * sizeof(pr_jpeg_sync_stats), s));
  if (a->n_segments > 0) {
    PR_HIP(hipMemsetAsync(p.owner, 0xFF, (size_t)l.T * 4, s));
    PR_HIP(hipMemsetAsync(p.changed, 0, (size_t)a->F * (R + 1) * 4, s));
    int cus = 0;
    PR_TRY(current_device_cus(&cus));
    p.lanes = (int)std::min((long)kSyncThreads, std::max(1l, ceil_div(l.T, (long)cus * PR_JPEG_SYNC_WAVES_PER_CU)));
    const dim3 per_segment((unsigned)ceil_div(a->n_segments, kSyncThreads)), per_lane((unsigned)ceil_div(l.T, (long)p.lanes));
    hipLaunchKernelGGL(jpeg_sync_map_kernel, per_segment, dim3(kSyncThreads), 0, s, p);
    PR_TRY(check_launch("jpeg_sync_map_kernel"));
    for (p.round = 0; p.round <= R; ++p.round) {
      hipLaunchKernelGGL(jpeg_sync_decode_kernel, per_lane, dim3(kSyncThreads), 0, s, p);
      PR_TRY(check_launch("jpeg_sync_decode_kernel"));
    }
    hipLaunchKernelGGL(jpeg_sync_scan_kernel, per_segment, dim3(kSyncThreads), 0, s, p);
    PR_TRY(check_launch("jpeg_sync_scan_kernel"));
    p.round = R + 1;
    hipLaunchKernelGGL(jpeg_sync_decode_kernel, per_lane, dim3(kSyncThreads), 0, s, p);
    PR_TRY(check_launch("jpeg_sync_decode_kernel"));
    PR_TRY(jpeg_launch_serial_entropy(p.j, s));
  }
  return jpeg_launch_back_end(p.j, s);
}
