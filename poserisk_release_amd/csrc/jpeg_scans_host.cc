// Host half of the multi-scan JPEG decoder (include/poserisk_hip.h, section j1b): pr_jpeg_parse with scans.  Marker parsing,
// the progression rules of T.81 G.1 as libjpeg enforces them, the scan / segment records and the levels pr_jpeg_decode_scans'
// kernels read.  Nothing is decoded here.  Device-free, as csrc/jpeg_host.cc: plain C++ under hipcc, g++ with
// -fsanitize=address,undefined for tests/native/jpeg_scans_native.cc.  Every read goes through Reader, which knows the file's
// end.  For a file pr_jpeg_parse accepts the frame and segment records written here are the ones it writes.
#include <algorithm>
#include <array>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "host_common.h"
#include "jpeg_host_tables.h"

namespace pr {
namespace {

const char* const kScanRefusal[PR_JPEG_E_SCAN_COUNT - PR_JPEG_E_COUNT] = {
    "a scan's spectral band or bit position is invalid (Ss > Se, Se > 63, Ah or Al > 13, or a progressive scan with Ss = 0 and "
    "Se != 0)",
    "an AC scan (Ss > 0) with more than one component",
    "the first scan of its coefficients has Ah != 0",
    "a refinement scan whose Ah is not the previous Al of the coefficients it covers, or whose Al is not Ah - 1",
    "an AC scan of a component before that component's first DC scan",
    "a refinement scan covers a coefficient that was never sent",
    "a component or coefficient is coded twice at one precision",
    "incomplete progression: at EOI a coefficient was never sent or has not reached Al = 0 (libjpeg would smooth such a file)",
};

typedef std::array<RawHuff, 4> RawSet;

struct ScanOut {
  pr_jpeg_segment* segs;
  int32_t* seg_scan;
  int seg_cap, n_segs = 0;
  pr_jpeg_huff* huff;
  int huff_cap, n_huff = 0;
  pr_jpeg_scan* scans;
  int scan_cap, n_scans = 0;
  int n_levels = 0, n_multi = 0;
  std::vector<uint64_t> huff_hash;
  std::vector<RawHuff> raw_sets;   // 4 per stored set: what the hash is checked against
};

// The index of `used` among the call's table sets, appended where it is new (-1 for counts that form no prefix code: parse_one
// has ruled that out before it calls).
int table_set(const RawHuff* used, ScanOut* o) {
  uint64_t h = 0;
  for (int i = 0; i < 4; ++i)
    if (used[i].defined) h = h * 31 + fnv(used[i].bits, 17) * 7 + fnv(used[i].vals, 256) + i;
  for (int i = o->n_huff - 1; i >= 0; --i)
    if (o->huff_hash[i] == h && same_raw(&o->raw_sets[4 * (size_t)i], used)) return i;
  pr_jpeg_huff built;
  memset(&built, 0, sizeof built);
  for (int i = 0; i < 4; ++i)
    if (used[i].defined && !build_table(used[i], &built.tab[i])) return -1;
  const int set = o->n_huff++;
  o->huff_hash.push_back(h);
  o->raw_sets.insert(o->raw_sets.end(), used, used + 4);
  if (set < o->huff_cap) o->huff[set] = built;
  return set;
}

// One file.  Returns PR_JPEG_OK or the refusal; on success *fr is filled and its scans, segments and table sets appended
// (counted even beyond the capacities, written only inside them).  A refused file appends nothing.
int parse_one(const uint8_t* data, int64_t begin, int64_t end, int frame_index, int* H, int* W, pr_jpeg_frame* fr, ScanOut* o) {
  Reader r{data, begin, end};
  if (!r.ok(2) || r.u8() != 0xFF || r.u8() != 0xD8) return PR_JPEG_E_NOT_JPEG;
  uint16_t qt[4][64];
  bool qt_defined[4] = {false, false, false, false};
  RawHuff huff[4];   // dc0, dc1, ac0, ac1
  bool have_sof = false, progressive = false;
  int comp_id[3] = {0, 0, 0}, comp_h[3] = {1, 1, 1}, comp_v[3] = {1, 1, 1}, comp_tq[3] = {0, 0, 0};
  int restart = 0;
  signed char al_of[3][64], level_of[3][64];   // per coefficient: the Al it stands at and the level that last wrote it; -1 = never sent
  memset(al_of, -1, sizeof al_of);
  memset(level_of, -1, sizeof level_of);
  bool seen[3] = {false, false, false};
  std::vector<pr_jpeg_scan> scans;
  std::vector<pr_jpeg_segment> segs;
  std::vector<int32_t> seg_scan;
  std::vector<RawSet> sets;
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
    if (m == 0xD9) {
      if (scans.empty()) return PR_JPEG_E_SCANS;   // EOI before any scan
      break;
    }
    if (m == 0x00 || m == 0x01 || (m >= 0xD0 && m <= 0xD8)) return PR_JPEG_E_MARKER;
    if (!r.ok(2)) return PR_JPEG_E_TRUNCATED;
    const int len = r.u16();
    if (len < 2) return PR_JPEG_E_MARKER;
    if (!r.ok(len - 2)) return PR_JPEG_E_TRUNCATED;
    const int64_t seg_end = r.pos + len - 2;
    Reader s{data, r.pos, seg_end};
    r.pos = seg_end;
    if (m == 0xC9 || m == 0xCA || m == 0xCB || m == 0xCD || m == 0xCE || m == 0xCF || m == 0xCC) return PR_JPEG_E_ARITHMETIC;
    if (m == 0xC1 || m == 0xC3 || m == 0xC5 || m == 0xC6 || m == 0xC7 || m == 0xC8) return PR_JPEG_E_EXTENDED;
    if (m == 0xDE || m == 0xDF || m == 0xDC) return PR_JPEG_E_EXTENDED;   // DHP, EXP, DNL
    if (m == 0xC0 || m == 0xC2) {
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
      progressive = m == 0xC2;
      continue;
    }
    if (m == 0xDB) {
      while (s.pos < s.end) {
        const int pq = s.u8();
        if ((pq >> 4) == 1) return PR_JPEG_E_QUANT16;
        if ((pq >> 4) != 0 || (pq & 15) > 3) return PR_JPEG_E_TABLE;
        if (!s.ok(64)) return PR_JPEG_E_MARKER;
        for (int k = 0; k < 64; ++k) qt[pq & 15][kZigzag[k]] = (uint16_t)s.u8();
        qt_defined[pq & 15] = true;
      }
      continue;
    }
    if (m == 0xC4) {
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
        if ((tc >> 4) == 0)   // a DC symbol is a bit count (csrc/jpeg_host.cc)
          for (int k = 0; k < total; ++k)
            if (t.vals[k] > 15) return PR_JPEG_E_TABLE;
        t.defined = true;
      }
      continue;
    }
    if (m == 0xDD) {
      if (s.end - s.pos != 2) return PR_JPEG_E_MARKER;
      restart = s.u16();
      continue;
    }
    if (m != 0xDA) continue;   // APPn, COM and anything else with a length: skipped

    // ---- a scan header --------------------------------------------------------------------------------------------------
    if (!have_sof) return PR_JPEG_E_MARKER;
    if (!s.ok(1)) return PR_JPEG_E_MARKER;
    const int ns = s.u8();
    if (ns < 1 || ns > fr->ncomp) return PR_JPEG_E_SCANS;
    if (s.end - s.pos != 2 * ns + 3) return PR_JPEG_E_MARKER;
    pr_jpeg_scan sc;
    memset(&sc, 0, sizeof sc);
    sc.frame = frame_index;
    sc.ncomp = ns;
    for (int i = 0; i < ns; ++i) {
      const int id = s.u8(), sel = s.u8();
      int c = 0;
      while (c < fr->ncomp && comp_id[c] != id) ++c;
      if (c == fr->ncomp || (i > 0 && c <= sc.comp[i - 1])) return PR_JPEG_E_SCANS;   // unknown, repeated or out of frame order
      if ((sel >> 4) > 1 || (sel & 15) > 1) return PR_JPEG_E_TABLE;
      sc.comp[i] = c;
      sc.dc_sel[i] = sel >> 4;
      sc.ac_sel[i] = sel & 15;
    }
    sc.ss = s.u8();
    sc.se = s.u8();
    const int ahal = s.u8();
    sc.ah = ahal >> 4;
    sc.al = ahal & 15;
    if (!progressive) {
      if (sc.ss != 0 || sc.se != 63 || ahal != 0) return PR_JPEG_E_PROGRESSIVE;
    } else {
      if (sc.ss > sc.se || sc.se > 63 || sc.ah > 13 || sc.al > 13 || (sc.ss == 0 && sc.se != 0)) return PR_JPEG_E_SCAN_BAND;
      if (sc.ss > 0 && ns > 1) return PR_JPEG_E_SCAN_AC_COMPONENTS;
      if (sc.ah != 0 && sc.al != sc.ah - 1) return PR_JPEG_E_SCAN_REFINE;
    }
    const bool needs_dc = sc.ss == 0 && sc.ah == 0, needs_ac = sc.se > 0;
    RawSet used;
    int level = 0;
    for (int i = 0; i < ns; ++i) {
      const int c = sc.comp[i];
      if (sc.ss > 0 && al_of[c][0] < 0) return PR_JPEG_E_SCAN_AC_BEFORE_DC;
      int sent = 0;
      for (int k = sc.ss; k <= sc.se; ++k) sent += al_of[c][k] >= 0;
      if (sc.ah == 0) {
        if (sent) return PR_JPEG_E_SCAN_TWICE;
      } else {
        if (!sent) return PR_JPEG_E_SCAN_FIRST_AH;
        if (sent != sc.se - sc.ss + 1) return PR_JPEG_E_SCAN_REFINE_UNSENT;
        for (int k = sc.ss; k <= sc.se; ++k) {
          if (al_of[c][k] == sc.al) return PR_JPEG_E_SCAN_TWICE;
          if (al_of[c][k] != sc.ah) return PR_JPEG_E_SCAN_REFINE;
        }
      }
      for (int k = sc.ss; k <= sc.se; ++k) {
        level = std::max(level, level_of[c][k] + 1);
        al_of[c][k] = (signed char)sc.al;
      }
      if ((needs_dc && !huff[sc.dc_sel[i]].defined) || (needs_ac && !huff[2 + sc.ac_sel[i]].defined)) return PR_JPEG_E_TABLE;
      if (needs_dc) used[sc.dc_sel[i]] = huff[sc.dc_sel[i]];
      if (needs_ac) used[2 + sc.ac_sel[i]] = huff[2 + sc.ac_sel[i]];
      if (!seen[c]) {   // the quantiser is latched at the component's first scan
        if (!qt_defined[comp_tq[c]]) return PR_JPEG_E_TABLE;
        memcpy(fr->quant[c], qt[comp_tq[c]], sizeof qt[0]);
        fr->dc_sel[c] = sc.dc_sel[i];
        fr->ac_sel[c] = sc.ac_sel[i];
        seen[c] = true;
      }
    }
    if (level >= PR_JPEG_MAX_LEVELS) return PR_JPEG_E_SCAN_REFINE;   // unreachable with Al <= 13; the device's bound
    for (int i = 0; i < ns; ++i)
      for (int k = sc.ss; k <= sc.se; ++k) level_of[sc.comp[i]][k] = (signed char)level;
    sc.level = level;
    sc.restart_interval = restart;
    if (ns > 1 || fr->ncomp == 1) {
      sc.n_mcus = ceil_div(fr->width, 8 * fr->hs) * ceil_div(fr->height, 8 * fr->vs);
    } else {   // one component of three: the blocks of its own size
      const int c = sc.comp[0];
      const int dw = c == 0 ? fr->width : ceil_div(fr->width, fr->hs), dh = c == 0 ? fr->height : ceil_div(fr->height, fr->vs);
      sc.n_mcus = ceil_div(dw, 8) * ceil_div(dh, 8);
    }

    // ---- its entropy-coded data: cut at RSTn, ended by the first other marker -----------------------------------------
    const int want = restart ? ceil_div(sc.n_mcus, restart) : 1;
    sc.first_segment = (int)segs.size();
    int found = 0;
    int64_t seg_begin = r.pos, pos = r.pos;
    int closing = -1;
    while (pos < end) {
      const uint8_t* ff = (const uint8_t*)memchr(data + pos, 0xFF, (size_t)(end - pos));
      if (!ff) break;
      pos = ff - data;
      if (pos + 1 >= end) break;                                  // a lone 0xFF at the end: truncated
      const int mk = data[pos + 1];
      if (mk == 0x00) { pos += 2; continue; }                     // a stuffed 0xFF data byte
      if (mk == 0xFF) { pos += 1; continue; }                     // a fill byte: the marker starts at the next 0xFF
      if (found >= want) return PR_JPEG_E_RESTARTS;
      pr_jpeg_segment sg;
      sg.begin = seg_begin;
      sg.end = pos;
      sg.frame = frame_index;
      sg.first_mcu = found * restart;
      segs.push_back(sg);
      seg_scan.push_back((int32_t)scans.size());
      ++found;
      if (mk >= 0xD0 && mk <= 0xD7) {
        if (!restart || mk != 0xD0 + ((found - 1) & 7)) return PR_JPEG_E_RESTARTS;
        pos += 2;
        seg_begin = pos;
        continue;
      }
      closing = mk;
      break;
    }
    if (closing < 0) return PR_JPEG_E_TRUNCATED;
    if (found != want) return PR_JPEG_E_RESTARTS;
    sc.n_segments = found;
    scans.push_back(sc);
    sets.push_back(used);
    r.pos = pos;   // the closing marker is read by the loop's head: EOI, or the tables and the header of the next scan
  }

  // ---- complete? ------------------------------------------------------------------------------------------------------------
  for (int c = 0; c < fr->ncomp; ++c)
    for (int k = 0; k < 64; ++k)
      if (al_of[c][k] != 0) return scans.size() == 1 && !progressive ? (int)PR_JPEG_E_SCANS : (int)PR_JPEG_E_SCAN_INCOMPLETE;
  // a call without a size takes it from the first frame that is ACCEPTED
  const bool adopt = *H == 0 && *W == 0;
  if (!adopt && (fr->height != *H || fr->width != *W)) return PR_JPEG_E_SIZE_DIFFERS;

  // ---- accepted: the table sets (stored once per distinct set of the call), then the records ----------------------------
  pr_jpeg_hufftab probe;
  for (const RawSet& set : sets)   // every table a prefix code, before anything is appended
    for (int i = 0; i < 4; ++i)
      if (set[i].defined && !build_table(set[i], &probe)) return PR_JPEG_E_TABLE;
  for (size_t i = 0; i < scans.size(); ++i) scans[i].huff_set = table_set(sets[i].data(), o);
  fr->restart_interval = scans[0].restart_interval;
  fr->huff_set = scans[0].huff_set;
  fr->first_segment = o->n_segs;
  fr->n_segments = (int)segs.size();
  int levels = 0;
  for (size_t i = 0; i < scans.size(); ++i) {
    scans[i].first_segment += o->n_segs;
    levels = std::max(levels, scans[i].level + 1);
    if (o->n_scans + (int)i < o->scan_cap) o->scans[o->n_scans + i] = scans[i];
  }
  for (size_t i = 0; i < segs.size(); ++i)
    if (o->n_segs + (int)i < o->seg_cap) {
      o->segs[o->n_segs + i] = segs[i];
      o->seg_scan[o->n_segs + i] = o->n_scans + seg_scan[i];
    }
  o->n_segs += (int)segs.size();
  o->n_scans += (int)scans.size();
  o->n_levels = std::max(o->n_levels, levels);
  o->n_multi += scans.size() > 1;
  if (adopt) {
    *H = fr->height;
    *W = fr->width;
  }
  return PR_JPEG_OK;
}

}  // namespace
}  // namespace pr

extern "C" const char* pr_jpeg_scan_refusal_name(int code) {
  if (code >= PR_JPEG_E_COUNT && code < PR_JPEG_E_SCAN_COUNT) return pr::kScanRefusal[code - PR_JPEG_E_COUNT];
  return pr_jpeg_refusal_name(code);
}

extern "C" int pr_jpeg_parse_scans(const uint8_t* data, const int64_t* offsets, int F, int H, int W, pr_jpeg_frame* frames,
                                   pr_jpeg_segment* segments, int32_t* segment_scan, int segment_capacity, pr_jpeg_huff* huff,
                                   int huff_capacity, pr_jpeg_scan* scans, int scan_capacity, int32_t* parse_status,
                                   int32_t* counts) {
  using namespace pr;
  PR_REQUIRE(F >= 0, "pr_jpeg_parse_scans: F = %d", F);
  PR_REQUIRE(counts, "pr_jpeg_parse_scans: null counts_host");
  PR_REQUIRE(segment_capacity >= 0 && huff_capacity >= 0 && scan_capacity >= 0,
             "pr_jpeg_parse_scans: negative capacity (%d segments, %d table sets, %d scans)", segment_capacity, huff_capacity,
             scan_capacity);
  PR_REQUIRE((H == 0 && W == 0) || (H >= 16 && H <= 4096 && W >= 16 && W <= 4096),
             "pr_jpeg_parse_scans: H x W = %d x %d is neither 0 x 0 nor inside 16..4096", H, W);
  memset(counts, 0, 8 * sizeof(int32_t));
  counts[2] = H;
  counts[3] = W;
  if (F == 0) return PR_OK;
  PR_REQUIRE(data, "pr_jpeg_parse_scans: null data_host");
  PR_REQUIRE(offsets, "pr_jpeg_parse_scans: null offsets_host");
  PR_REQUIRE(frames, "pr_jpeg_parse_scans: null frames_host");
  PR_REQUIRE(parse_status, "pr_jpeg_parse_scans: null parse_status_host");
  PR_REQUIRE((segments && segment_scan) || segment_capacity == 0,
             "pr_jpeg_parse_scans: null segments_host or segment_scan_host with capacity %d", segment_capacity);
  PR_REQUIRE(huff || huff_capacity == 0, "pr_jpeg_parse_scans: null huff_host with capacity %d", huff_capacity);
  PR_REQUIRE(scans || scan_capacity == 0, "pr_jpeg_parse_scans: null scans_host with capacity %d", scan_capacity);
  PR_REQUIRE(offsets[0] >= 0, "pr_jpeg_parse_scans: offsets_host[0] = %lld", (long long)offsets[0]);
  for (int f = 0; f < F; ++f)
    PR_REQUIRE(offsets[f + 1] >= offsets[f], "pr_jpeg_parse_scans: offsets_host[%d] = %lld is below offsets_host[%d] = %lld",
               f + 1, (long long)offsets[f + 1], f, (long long)offsets[f]);
  ScanOut o;
  o.segs = segments;
  o.seg_scan = segment_scan;
  o.seg_cap = segment_capacity;
  o.huff = huff;
  o.huff_cap = huff_capacity;
  o.scans = scans;
  o.scan_cap = scan_capacity;
  for (int f = 0; f < F; ++f) {
    const int st = parse_one(data, offsets[f], offsets[f + 1], f, &H, &W, &frames[f], &o);
    parse_status[f] = st;
    if (st != PR_JPEG_OK) {
      memset(&frames[f], 0, sizeof frames[f]);   // ncomp = 0: the device zero-fills this frame
      frames[f].first_segment = o.n_segs;
      set_error("pr_jpeg_parse_scans: frame %d refused: %s", f, pr_jpeg_scan_refusal_name(st));
    }
  }
  counts[0] = o.n_segs;
  counts[1] = o.n_huff;
  counts[2] = H;
  counts[3] = W;
  counts[4] = o.n_scans;
  counts[5] = o.n_levels;
  counts[6] = o.n_multi;
  if (o.n_segs > segment_capacity || o.n_huff > huff_capacity || o.n_scans > scan_capacity) {
    set_error("pr_jpeg_parse_scans: %d segments, %d table sets and %d scans are needed, room for %d, %d and %d was given",
              o.n_segs, o.n_huff, o.n_scans, segment_capacity, huff_capacity, scan_capacity);
    return PR_ERR_CAPACITY;
  }
  return PR_OK;
}
