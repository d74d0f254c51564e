// Host half of the JPEG decoder (include/poserisk_hip.h, section j1): marker parsing, validation and the per-frame
// descriptors pr_jpeg_decode's kernels read.  Nothing is decoded here.  Behind it, the encoder's host half (section j2):
// pr_jpeg_encode_plan derives the tables and the header bytes pr_jpeg_encode's kernels read, pr_jpeg_encode_bound the size no
// file exceeds.  Device-free: compiled into libposerisk_hip.so by
// hipcc as plain C++ and, for the tests/native/jpeg*_native.cc drivers, by g++ with -fsanitize=address,undefined.  No HIP header may be
// included here.  Every read goes through Reader, which knows the file's end: a stream cut or corrupted anywhere ends in a
// refusal or in descriptors whose ranges lie inside the file.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <vector>

#include "host_common.h"
#include "jpeg_host_tables.h"

namespace pr {
namespace {

const char* const kRefusal[PR_JPEG_E_COUNT] = {
    "ok",
    "not a JPEG stream (no SOI marker)",
    "truncated (the stream ends before EOI)",
    "progressive JPEG (SOF2) is not supported",
    "extended, lossless or hierarchical JPEG (SOF1, SOF3, SOF5..15) is not supported",
    "arithmetic coding is not supported",
    "sample precision other than 8 bits is not supported",
    "component count other than 1 or 3 is not supported",
    "sampling other than luma 1x1 / 2x1 / 2x2 with chroma 1x1 is not supported",
    "more than one scan, or a scan that does not interleave all components, is not supported",
    "16-bit quantisation tables are not supported",
    "width or height outside 16..4096",
    "frame size differs from the other frames of the call",
    "a missing or invalid quantisation or Huffman table, or a table id above 1",
    "an invalid or unexpected marker segment",
    "the restart markers do not match the restart interval",
};

struct Out {
  pr_jpeg_segment* segs;
  int seg_cap, n_segs = 0;
  pr_jpeg_huff* huff;
  int huff_cap, n_huff = 0;
  std::vector<uint64_t> huff_hash;
  std::vector<RawHuff> raw_sets;   // 4 per stored set: what the hash is checked against
};

// One file.  Returns PR_JPEG_OK or the refusal; on success *fr is filled and its segments appended (counted even beyond the
// capacity, written only inside it).
int parse_one(const uint8_t* data, int64_t begin, int64_t end, int frame_index, int* H, int* W, pr_jpeg_frame* fr, Out* o) {
  Reader r{data, begin, end};
  if (!r.ok(2) || r.u8() != 0xFF || r.u8() != 0xD8) return PR_JPEG_E_NOT_JPEG;
  uint16_t qt[4][64];
  bool qt_defined[4] = {false, false, false, false};
  RawHuff huff[4];   // dc0, dc1, ac0, ac1
  bool have_sof = false;
  int comp_id[3] = {0, 0, 0}, comp_h[3] = {1, 1, 1}, comp_v[3] = {1, 1, 1}, comp_tq[3] = {0, 0, 0};
  int restart = 0;
  memset(fr, 0, sizeof *fr);
  for (;;) {
    // a marker: 0xFF, any number of 0xFF fill bytes, the code
    if (!r.ok(2)) return PR_JPEG_E_TRUNCATED;
    if (r.u8() != 0xFF) return PR_JPEG_E_MARKER;
    int m = r.u8();
    while (m == 0xFF) {
      if (!r.ok(1)) return PR_JPEG_E_TRUNCATED;
      m = r.u8();
    }
    if (m == 0xD9) return PR_JPEG_E_SCANS;                     // EOI before any scan
    if (m == 0x00 || m == 0x01 || (m >= 0xD0 && m <= 0xD8)) return PR_JPEG_E_MARKER;
    if (!r.ok(2)) return PR_JPEG_E_TRUNCATED;
    const int len = r.u16();
    if (len < 2) return PR_JPEG_E_MARKER;
    if (!r.ok(len - 2)) return PR_JPEG_E_TRUNCATED;
    const int64_t seg_end = r.pos + len - 2;
    Reader s{data, r.pos, seg_end};
    r.pos = seg_end;
    if (m == 0xC2) return PR_JPEG_E_PROGRESSIVE;
    if (m == 0xC9 || m == 0xCA || m == 0xCB || m == 0xCD || m == 0xCE || m == 0xCF || m == 0xCC) return PR_JPEG_E_ARITHMETIC;
    if (m == 0xC1 || m == 0xC3 || m == 0xC5 || m == 0xC6 || m == 0xC7 || m == 0xC8) return PR_JPEG_E_EXTENDED;
    if (m == 0xDE || m == 0xDF || m == 0xDC) return PR_JPEG_E_EXTENDED;   // DHP, EXP, DNL
    if (m == 0xC0) {
      if (have_sof) return PR_JPEG_E_MARKER;
      if (!s.ok(6)) return PR_JPEG_E_MARKER;
      const int prec = s.u8(), h = s.u16(), w = s.u16(), nc = s.u8();
      if (prec != 8) return PR_JPEG_E_PRECISION;
      if (nc != 1 && nc != 3) return PR_JPEG_E_COMPONENTS;
      if (h < 16 || w < 16 || h > 4096 || w > 4096) return PR_JPEG_E_DIMENSIONS;
      if (!s.ok(3 * nc) || s.end - s.pos != 3 * nc) return PR_JPEG_E_MARKER;
      for (int c = 0; c < nc; ++c) {
        comp_id[c] = s.u8();
        const int hv = s.u8();
        comp_h[c] = hv >> 4;
        comp_v[c] = hv & 15;
        comp_tq[c] = s.u8();
        if (comp_h[c] < 1 || comp_h[c] > 4 || comp_v[c] < 1 || comp_v[c] > 4) return PR_JPEG_E_SAMPLING;
        if (comp_tq[c] > 3) return PR_JPEG_E_TABLE;
        for (int d = 0; d < c; ++d)
          if (comp_id[d] == comp_id[c]) return PR_JPEG_E_MARKER;
      }
      if (nc == 3) {
        const bool luma_ok = (comp_h[0] == 1 && comp_v[0] == 1) || (comp_h[0] == 2 && comp_v[0] == 1) ||
                             (comp_h[0] == 2 && comp_v[0] == 2);
        if (!luma_ok || comp_h[1] != 1 || comp_v[1] != 1 || comp_h[2] != 1 || comp_v[2] != 1) return PR_JPEG_E_SAMPLING;
      }
      fr->width = w;
      fr->height = h;
      fr->ncomp = nc;
      fr->hs = nc == 3 ? comp_h[0] : 1;
      fr->vs = nc == 3 ? comp_v[0] : 1;
      have_sof = true;
    } else if (m == 0xDB) {
      while (s.pos < s.end) {
        const int pq = s.u8();
        if ((pq >> 4) == 1) return PR_JPEG_E_QUANT16;
        if ((pq >> 4) != 0 || (pq & 15) > 3) return PR_JPEG_E_TABLE;
        if (!s.ok(64)) return PR_JPEG_E_MARKER;
        for (int k = 0; k < 64; ++k) qt[pq & 15][kZigzag[k]] = (uint16_t)s.u8();
        qt_defined[pq & 15] = true;
      }
    } else if (m == 0xC4) {
      while (s.pos < s.end) {
        const int tc = s.u8();
        if ((tc >> 4) > 1 || (tc & 15) > 1) return PR_JPEG_E_TABLE;
        RawHuff& t = huff[(tc >> 4) * 2 + (tc & 15)];
        if (!s.ok(16)) return PR_JPEG_E_MARKER;
        int total = 0;
        t = RawHuff();
        for (int l = 1; l <= 16; ++l) total += (t.bits[l] = (uint8_t)s.u8());
        if (total > 256 || !s.ok(total)) return PR_JPEG_E_TABLE;
        for (int k = 0; k < total; ++k) t.vals[k] = (uint8_t)s.u8();
        // a DC symbol is a bit count: above 11 no 8-bit stream has one, above 16 receive-and-extend has no meaning
        if ((tc >> 4) == 0)
          for (int k = 0; k < total; ++k)
            if (t.vals[k] > 15) return PR_JPEG_E_TABLE;
        t.defined = true;
      }
    } else if (m == 0xDD) {
      if (s.end - s.pos != 2) return PR_JPEG_E_MARKER;
      restart = s.u16();
    } else if (m == 0xDA) {
      if (!have_sof) return PR_JPEG_E_MARKER;
      if (!s.ok(1)) return PR_JPEG_E_MARKER;
      const int ns = s.u8();
      if (ns != fr->ncomp) return PR_JPEG_E_SCANS;
      if (s.end - s.pos != 2 * ns + 3) return PR_JPEG_E_MARKER;
      for (int c = 0; c < ns; ++c) {
        const int id = s.u8(), sel = s.u8();
        if (id != comp_id[c]) return PR_JPEG_E_SCANS;
        if ((sel >> 4) > 1 || (sel & 15) > 1) return PR_JPEG_E_TABLE;
        fr->dc_sel[c] = sel >> 4;
        fr->ac_sel[c] = sel & 15;
        if (!huff[fr->dc_sel[c]].defined || !huff[2 + fr->ac_sel[c]].defined || !qt_defined[comp_tq[c]]) return PR_JPEG_E_TABLE;
        memcpy(fr->quant[c], qt[comp_tq[c]], sizeof qt[0]);
      }
      const int ss = s.u8(), se = s.u8(), ahal = s.u8();
      if (ss != 0 || se != 63 || ahal != 0) return PR_JPEG_E_PROGRESSIVE;
      break;
    }
    // APPn, COM and anything else with a length: skipped
  }
  // a call without a size takes it from the first frame that is ACCEPTED: adopted at the end, once nothing can refuse it
  const bool adopt = *H == 0 && *W == 0;
  if (!adopt && (fr->height != *H || fr->width != *W)) return PR_JPEG_E_SIZE_DIFFERS;

  // ---- the entropy-coded data: cut at RSTn, ended by the first other marker ------------------------------------------------
  const int mcus = ceil_div(fr->width, 8 * fr->hs) * ceil_div(fr->height, 8 * fr->vs);
  const int want = restart ? ceil_div(mcus, restart) : 1;
  fr->restart_interval = restart;
  fr->first_segment = o->n_segs;
  int found = 0;
  int64_t seg_begin = r.pos, pos = r.pos;
  int closing = -1;
  while (pos < end) {
    const uint8_t* ff = (const uint8_t*)memchr(data + pos, 0xFF, (size_t)(end - pos));
    if (!ff) break;
    pos = ff - data;
    if (pos + 1 >= end) break;                                  // a lone 0xFF at the end: truncated
    const int m = data[pos + 1];
    if (m == 0x00) { pos += 2; continue; }                      // a stuffed 0xFF data byte
    if (m == 0xFF) { pos += 1; continue; }                      // a fill byte: the marker starts at the next 0xFF
    // a marker ends the segment in front of it
    if (found >= want) return PR_JPEG_E_RESTARTS;
    if (o->n_segs + found < o->seg_cap) {
      pr_jpeg_segment& sg = o->segs[o->n_segs + found];
      sg.begin = seg_begin;
      sg.end = pos;
      sg.frame = frame_index;
      sg.first_mcu = found * restart;
    }
    ++found;
    if (m >= 0xD0 && m <= 0xD7) {
      if (!restart || m != 0xD0 + ((found - 1) & 7)) return PR_JPEG_E_RESTARTS;
      pos += 2;
      seg_begin = pos;
      continue;
    }
    closing = m;
    break;
  }
  if (closing < 0) return PR_JPEG_E_TRUNCATED;
  if (closing == 0xDA || closing == 0xC4 || closing == 0xDB || closing == 0xDD) return PR_JPEG_E_SCANS;
  if (closing != 0xD9) return PR_JPEG_E_MARKER;
  if (found != want) return PR_JPEG_E_RESTARTS;
  fr->n_segments = found;

  // ---- the table set, stored once per distinct set of the call ---------------------------------------------------------
  RawHuff used[4];
  for (int c = 0; c < fr->ncomp; ++c) {
    used[fr->dc_sel[c]] = huff[fr->dc_sel[c]];
    used[2 + fr->ac_sel[c]] = huff[2 + fr->ac_sel[c]];
  }
  uint64_t h = 0;
  for (int i = 0; i < 4; ++i)
    if (used[i].defined) h = h * 31 + fnv(used[i].bits, 17) * 7 + fnv(used[i].vals, 256) + i;
  int set = -1;
  for (int i = o->n_huff - 1; i >= 0 && set < 0; --i)
    if (o->huff_hash[i] == h && same_raw(&o->raw_sets[4 * (size_t)i], used)) set = i;
  if (set < 0) {
    pr_jpeg_huff built;
    memset(&built, 0, sizeof built);
    for (int i = 0; i < 4; ++i)
      if (used[i].defined && !build_table(used[i], &built.tab[i])) return PR_JPEG_E_TABLE;
    set = o->n_huff++;
    o->huff_hash.push_back(h);
    o->raw_sets.insert(o->raw_sets.end(), used, used + 4);
    if (set < o->huff_cap) o->huff[set] = built;
  }
  fr->huff_set = set;
  o->n_segs += found;
  if (adopt) {
    *H = fr->height;
    *W = fr->width;
  }
  return PR_JPEG_OK;
}

}  // namespace
}  // namespace pr

extern "C" const char* pr_jpeg_refusal_name(int code) {
  return code >= 0 && code < PR_JPEG_E_COUNT ? pr::kRefusal[code] : "unknown refusal code";
}

extern "C" int pr_jpeg_parse(const uint8_t* data, const int64_t* offsets, int F, int H, int W, pr_jpeg_frame* frames,
                             pr_jpeg_segment* segments, int segment_capacity, pr_jpeg_huff* huff, int huff_capacity,
                             int32_t* parse_status, int32_t* counts) {
  using namespace pr;
  PR_REQUIRE(F >= 0, "pr_jpeg_parse: F = %d", F);
  PR_REQUIRE(counts, "pr_jpeg_parse: null counts_host");
  PR_REQUIRE(segment_capacity >= 0 && huff_capacity >= 0, "pr_jpeg_parse: negative capacity (%d segments, %d table sets)",
             segment_capacity, huff_capacity);
  PR_REQUIRE((H == 0 && W == 0) || (H >= 16 && H <= 4096 && W >= 16 && W <= 4096),
             "pr_jpeg_parse: H x W = %d x %d is neither 0 x 0 nor inside 16..4096", H, W);
  counts[0] = counts[1] = 0;
  counts[2] = H;
  counts[3] = W;
  if (F == 0) return PR_OK;
  PR_REQUIRE(data, "pr_jpeg_parse: null data_host");
  PR_REQUIRE(offsets, "pr_jpeg_parse: null offsets_host");
  PR_REQUIRE(frames, "pr_jpeg_parse: null frames_host");
  PR_REQUIRE(parse_status, "pr_jpeg_parse: null parse_status_host");
  PR_REQUIRE(segments || segment_capacity == 0, "pr_jpeg_parse: null segments_host with capacity %d", segment_capacity);
  PR_REQUIRE(huff || huff_capacity == 0, "pr_jpeg_parse: null huff_host with capacity %d", huff_capacity);
  PR_REQUIRE(offsets[0] >= 0, "pr_jpeg_parse: offsets_host[0] = %lld", (long long)offsets[0]);
  for (int f = 0; f < F; ++f)
    PR_REQUIRE(offsets[f + 1] >= offsets[f], "pr_jpeg_parse: offsets_host[%d] = %lld is below offsets_host[%d] = %lld", f + 1,
               (long long)offsets[f + 1], f, (long long)offsets[f]);
  Out o;
  o.segs = segments;
  o.seg_cap = segment_capacity;
  o.huff = huff;
  o.huff_cap = huff_capacity;
  for (int f = 0; f < F; ++f) {
    const int segs_before = o.n_segs;
    const int st = parse_one(data, offsets[f], offsets[f + 1], f, &H, &W, &frames[f], &o);
    parse_status[f] = st;
    if (st != PR_JPEG_OK) {
      memset(&frames[f], 0, sizeof frames[f]);   // ncomp = 0: the device zero-fills this frame
      frames[f].first_segment = o.n_segs = segs_before;
      set_error("pr_jpeg_parse: frame %d refused: %s", f, pr_jpeg_refusal_name(st));
    }
  }
  counts[0] = o.n_segs;
  counts[1] = o.n_huff;
  counts[2] = H;
  counts[3] = W;
  if (o.n_segs > segment_capacity || o.n_huff > huff_capacity) {
    set_error("pr_jpeg_parse: %d segments and %d table sets are needed, room for %d and %d was given", o.n_segs, o.n_huff,
              segment_capacity, huff_capacity);
    return PR_ERR_CAPACITY;
  }
  return PR_OK;
}

// ---- the encoder's host half (include/poserisk_hip.h, section j2) ------------------------------------------------------------
namespace pr {
namespace {

// Annex K.1, natural order
const uint8_t kBaseQuant[2][64] = {
    {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
     18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112,
     100, 103, 99},
    {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};
// Annex K.3: code counts per length 1..16, then the symbols in code order
const uint8_t kDcBits[2][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}};
const uint8_t kDcVals[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
const uint8_t kAcBits[2][16] = {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d}, {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77}};
const uint8_t kAcVals[2][162] = {
    {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81,
     0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18,
     0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48,
     0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75,
     0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99,
     0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
     0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5,
     0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa},
    {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08,
     0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25,
     0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47,
     0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74,
     0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97,
     0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba,
     0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4,
     0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa}};

// MCUs per restart segment as libjpeg keeps it (0 = none), or -2 for parameters the encoder does not accept
int enc_restart(int H, int W, int hs, int vs, int restart_interval) {
  const bool sampling = (hs == 1 && vs == 1) || (hs == 2 && vs == 1) || (hs == 2 && vs == 2);
  if (!sampling || H < 16 || W < 16 || H > 4096 || W > 4096 || restart_interval < -1) return -2;
  const int ri = restart_interval < 0 ? (W + 8 * hs - 1) / (8 * hs) : restart_interval;
  return std::min(ri, 65535);
}

void enc_codes(const uint8_t* bits, const uint8_t* vals, uint16_t* code_of, uint8_t* len_of) {
  int code = 0, k = 0;
  for (int l = 1; l <= 16; ++l) {
    for (int i = 0; i < bits[l - 1]; ++i, ++code, ++k) {
      code_of[vals[k]] = (uint16_t)code;
      len_of[vals[k]] = (uint8_t)l;
    }
    code <<= 1;
  }
}

}  // namespace

// ceil(2^32 / q8) for q8 = 8..2040: the multiplier pr_jpeg_encode's quantiser uses in place of the division
uint32_t enc_recip(uint32_t q8) { return (uint32_t)(((1ull << 32) + q8 - 1) / q8); }

}  // namespace pr

extern "C" size_t pr_jpeg_encode_bound(int H, int W, int hs, int vs, int restart_interval) {
  const int ri = pr::enc_restart(H, W, hs, vs, restart_interval);
  if (ri < 0) return 0;
  const size_t mcus = (size_t)((W + 8 * hs - 1) / (8 * hs)) * (size_t)((H + 8 * vs - 1) / (8 * vs));
  const size_t segs = ri ? (mcus + ri - 1) / ri : 1;
  const size_t head = 623 + (ri ? 6 : 0);
  return head + mcus * (hs * vs + 2) * PR_JPEG_ENC_BLOCK_BITS / 4 + 4 * segs + 2;
}

extern "C" int pr_jpeg_encode_plan(int quality, int hs, int vs, int restart_interval, int H, int W, pr_jpeg_enc_plan* plan) {
  using namespace pr;
  PR_REQUIRE(plan, "pr_jpeg_encode_plan: null plan_host");
  PR_REQUIRE(quality >= 1 && quality <= 100, "pr_jpeg_encode_plan: quality = %d outside 1..100", quality);
  const int ri = enc_restart(H, W, hs, vs, restart_interval);
  PR_REQUIRE(ri >= 0,
             "pr_jpeg_encode_plan: %d x %d frames, sampling %d x %d, restart interval %d: sizes are 16..4096, sampling 1x1, 2x1 or "
             "2x2, the interval -1, 0 or a count of MCUs", W, H, hs, vs, restart_interval);
  memset(plan, 0, sizeof *plan);
  plan->width = W;
  plan->height = H;
  plan->hs = hs;
  plan->vs = vs;
  plan->restart_interval = ri;
  plan->quality = quality;
  const int scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;
  for (int t = 0; t < 2; ++t) {
    for (int i = 0; i < 64; ++i) {
      const int q = std::min(255, std::max(1, (kBaseQuant[t][i] * scale + 50) / 100));
      plan->quant[t][i] = (uint16_t)q;
      plan->recip[t][i] = enc_recip(8u * q);
    }
    enc_codes(kDcBits[t], kDcVals, plan->dc_code[t], plan->dc_len[t]);
    enc_codes(kAcBits[t], kAcVals[t], plan->ac_code[t], plan->ac_len[t]);
  }
  uint8_t* h = plan->header;
  int n = 0;
  auto put = [&](std::initializer_list<int> bytes) {
    for (int b : bytes) h[n++] = (uint8_t)b;
  };
  put({0xFF, 0xD8, 0xFF, 0xE0, 0, 16, 'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0});
  for (int t = 0; t < 2; ++t) {
    put({0xFF, 0xDB, 0, 67, t});
    for (int i = 0; i < 64; ++i) h[n++] = (uint8_t)plan->quant[t][kZigzag[i]];
  }
  put({0xFF, 0xC0, 0, 17, 8, H >> 8, H & 255, W >> 8, W & 255, 3, 1, hs << 4 | vs, 0, 2, 0x11, 1, 3, 0x11, 1});
  for (int t = 0; t < 2; ++t) {
    put({0xFF, 0xC4, 0, 2 + 1 + 16 + 12, t});
    for (int i = 0; i < 16; ++i) h[n++] = kDcBits[t][i];
    for (int i = 0; i < 12; ++i) h[n++] = kDcVals[i];
    put({0xFF, 0xC4, 0, 2 + 1 + 16 + 162, 0x10 | t});
    for (int i = 0; i < 16; ++i) h[n++] = kAcBits[t][i];
    for (int i = 0; i < 162; ++i) h[n++] = kAcVals[t][i];
  }
  if (ri) put({0xFF, 0xDD, 0, 4, ri >> 8, ri & 255});
  put({0xFF, 0xDA, 0, 12, 3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0});
  plan->header_bytes = n;
  return PR_OK;
}
