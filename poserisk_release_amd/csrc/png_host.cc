// Host half of the PNG decoder (include/poserisk_hip.h, section j4): the chunk walk.  Device-free, like jpeg_host.cc: it is
// compiled without the offload pass, and by g++ under sanitizers for tests/test_png_native.py.  It checks the signature,
// every chunk's CRC-32, IHDR and the zlib header and emits DESCRIPTORS ONLY -- a pr_png_frame per file, a (begin, end) range
// into the caller's bytes per IDAT chunk, a padded palette -- so that nothing but the files' own bytes and these records
// crosses to the device.  tests/png_ref.py restates the walk in Python.
#include "host_common.h"

namespace pr {
namespace {

const char* const kPngRefusal[PR_PNG_E_COUNT] = {
    "ok",
    "not a PNG file (no PNG signature)",
    "the file ends inside a chunk",
    "a chunk's CRC-32 does not match",
    "IHDR, PLTE, IDAT or IEND is missing or misplaced",
    "16-bit samples are not supported",
    "bit depths 1, 2 and 4 are not supported",
    "Adam7 interlace is not supported",
    "Apple's CgBI variant is not a PNG",
    "IHDR holds a depth, colour type, method or size no PNG of this decoder has",
    "its size differs from the other frames of the call",
    "the zlib header is not deflate with a window of at most 32 KiB, no dictionary and a valid check",
};

// CRC-32 by slicing: eight table look-ups per eight bytes (the byte-at-a-time loop was the whole decode's bound on the host:
// every byte of every file goes through here once).
struct Crc {
  uint32_t t[8][256];
  Crc() {
    for (uint32_t n = 0; n < 256; ++n) {
      uint32_t c = n;
      for (int k = 0; k < 8; ++k) c = (c & 1) ? 0xEDB88320u ^ (c >> 1) : c >> 1;
      t[0][n] = c;
    }
    for (uint32_t n = 0; n < 256; ++n)
      for (int k = 1; k < 8; ++k) t[k][n] = t[0][t[k - 1][n] & 255] ^ (t[k - 1][n] >> 8);
  }
  uint32_t of(const uint8_t* p, int64_t n) const {
    uint32_t c = 0xFFFFFFFFu;
    int64_t i = 0;
    for (; i + 8 <= n; i += 8) {
      const uint32_t lo = c ^ ((uint32_t)p[i] | (uint32_t)p[i + 1] << 8 | (uint32_t)p[i + 2] << 16 | (uint32_t)p[i + 3] << 24);
      c = t[7][lo & 255] ^ t[6][lo >> 8 & 255] ^ t[5][lo >> 16 & 255] ^ t[4][lo >> 24] ^ t[3][p[i + 4]] ^ t[2][p[i + 5]] ^ t[1][p[i + 6]] ^
          t[0][p[i + 7]];
    }
    for (; i < n; ++i) c = t[0][(c ^ p[i]) & 255] ^ (c >> 8);
    return ~c;
  }
};

inline uint32_t be32(const uint8_t* p) { return (uint32_t)p[0] << 24 | (uint32_t)p[1] << 16 | (uint32_t)p[2] << 8 | p[3]; }

struct Out {
  pr_png_idat* idat;
  int idat_cap, n_idat = 0;
  uint8_t* palettes;
  int pal_cap, n_pal = 0;
};

// One file, bytes [b, e) of data.  Ranges and the palette are written only where there is room; the counts go on.
int parse_one(const uint8_t* data, int64_t b, int64_t e, int* H, int* W, pr_png_frame* fr, Out* o) {
  static const Crc crc;
  static const uint8_t kSig[8] = {0x89, 'P', 'N', 'G', '\r', '\n', 0x1A, '\n'};
  if (e - b < 8 || memcmp(data + b, kSig, 8) != 0) return PR_PNG_E_SIGNATURE;
  int64_t p = b + 8;
  bool have_ihdr = false, have_plte = false, in_idat = false, idat_done = false, have_iend = false;
  uint8_t zhead[2] = {0, 0};
  int64_t zbytes = 0;
  memset(fr, 0, sizeof *fr);
  fr->palette = -1;
  fr->first_idat = o->n_idat;
  while (!have_iend) {
    if (e - p < 12) return PR_PNG_E_TRUNCATED;
    const int64_t len = be32(data + p);
    if (len > e - p - 12) return PR_PNG_E_TRUNCATED;
    const uint8_t* type = data + p + 4;
    const uint8_t* body = data + p + 8;
    const bool first = p == b + 8;
    if (first && memcmp(type, "CgBI", 4) == 0) return PR_PNG_E_CGBI;
    if (crc.of(type, 4 + len) != be32(body + len)) return PR_PNG_E_CRC;
    const bool is_idat = memcmp(type, "IDAT", 4) == 0;
    if (in_idat && !is_idat) {
      in_idat = false;
      idat_done = true;
    }
    if (memcmp(type, "IHDR", 4) == 0) {
      if (!first || len != 13) return PR_PNG_E_CHUNK_ORDER;
      have_ihdr = true;
      const uint32_t w = be32(body), h = be32(body + 4);
      const int depth = body[8], ct = body[9];
      if (!(ct == 0 || ct == 2 || ct == 3 || ct == 4 || ct == 6)) return PR_PNG_E_IHDR;
      if (depth == 16) return ct == 3 ? PR_PNG_E_IHDR : PR_PNG_E_DEPTH16;
      if (depth == 1 || depth == 2 || depth == 4) return (ct == 0 || ct == 3) ? PR_PNG_E_DEPTH_SUB8 : PR_PNG_E_IHDR;
      if (depth != 8 || body[10] != 0 || body[11] != 0) return PR_PNG_E_IHDR;
      if (body[12] == 1) return PR_PNG_E_INTERLACE;
      if (body[12] != 0) return PR_PNG_E_IHDR;
      if (w == 0 || h == 0 || w > PR_PNG_MAX_SIDE || h > PR_PNG_MAX_SIDE) return PR_PNG_E_IHDR;
      fr->width = (int32_t)w;
      fr->height = (int32_t)h;
      fr->color_type = ct;
      fr->bpp = ct == 0 ? 1 : ct == 2 ? 3 : ct == 3 ? 1 : ct == 4 ? 2 : 4;
    } else if (first) {
      return PR_PNG_E_CHUNK_ORDER;   // something else in IHDR's place
    } else if (memcmp(type, "PLTE", 4) == 0) {
      if (have_plte || in_idat || idat_done || len == 0 || len > 768 || len % 3 != 0 || fr->color_type == 0 || fr->color_type == 4)
        return PR_PNG_E_CHUNK_ORDER;
      have_plte = true;
      if (fr->color_type == 3) {
        fr->palette = o->n_pal;
        if (o->n_pal < o->pal_cap) {
          uint8_t* dst = o->palettes + (size_t)o->n_pal * 768;
          memset(dst, 0, 768);
          memcpy(dst, body, (size_t)len);
        }
        ++o->n_pal;
      }
    } else if (is_idat) {
      if (idat_done || (fr->color_type == 3 && !have_plte)) return PR_PNG_E_CHUNK_ORDER;
      in_idat = true;
      for (int64_t i = 0; i < len && zbytes + i < 2; ++i) zhead[zbytes + i] = body[i];
      zbytes += len;
      if (o->n_idat < o->idat_cap) {
        o->idat[o->n_idat].begin = (body - data);
        o->idat[o->n_idat].end = (body - data) + len;
      }
      ++o->n_idat;
      ++fr->n_idat;
    } else if (memcmp(type, "IEND", 4) == 0) {
      if (len != 0) return PR_PNG_E_CHUNK_ORDER;
      have_iend = true;
    }
    p += 12 + len;
  }
  if (!have_ihdr || fr->n_idat == 0) return PR_PNG_E_CHUNK_ORDER;
  if (zbytes < 2 || (zhead[0] & 15) != 8 || (zhead[0] >> 4) > 7 || (zhead[1] & 32) || (zhead[0] * 256 + zhead[1]) % 31 != 0)
    return PR_PNG_E_ZLIB_HEADER;
  fr->zlib_bytes = zbytes;
  if (*H == 0 && *W == 0) {
    *H = fr->height;
    *W = fr->width;
  } else if (fr->height != *H || fr->width != *W) {
    return PR_PNG_E_SIZE_DIFFERS;
  }
  return PR_PNG_OK;
}

}  // namespace
}  // namespace pr

extern "C" const char* pr_png_refusal_name(int code) {
  return code >= 0 && code < PR_PNG_E_COUNT ? pr::kPngRefusal[code] : "unknown refusal code";
}

extern "C" int pr_png_parse(const uint8_t* data, const int64_t* offsets, int F, int H, int W, pr_png_frame* frames, pr_png_idat* idat,
                            int idat_capacity, uint8_t* palettes, int palette_capacity, int32_t* parse_status, int32_t* counts) {
  using namespace pr;
  PR_REQUIRE(F >= 0, "pr_png_parse: F = %d", F);
  PR_REQUIRE(counts, "pr_png_parse: null counts_host");
  PR_REQUIRE(idat_capacity >= 0 && palette_capacity >= 0, "pr_png_parse: negative capacity (%d ranges, %d palettes)", idat_capacity,
             palette_capacity);
  PR_REQUIRE((H == 0 && W == 0) || (H >= 1 && H <= PR_PNG_MAX_SIDE && W >= 1 && W <= PR_PNG_MAX_SIDE),
             "pr_png_parse: H x W = %d x %d is neither 0 x 0 nor inside 1..%d", H, W, PR_PNG_MAX_SIDE);
  counts[0] = counts[1] = 0;
  counts[2] = H;
  counts[3] = W;
  if (F == 0) return PR_OK;
  PR_REQUIRE(data, "pr_png_parse: null data_host");
  PR_REQUIRE(offsets, "pr_png_parse: null offsets_host");
  PR_REQUIRE(frames, "pr_png_parse: null frames_host");
  PR_REQUIRE(parse_status, "pr_png_parse: null parse_status_host");
  PR_REQUIRE(idat || idat_capacity == 0, "pr_png_parse: null idat_host with capacity %d", idat_capacity);
  PR_REQUIRE(palettes || palette_capacity == 0, "pr_png_parse: null palettes_host with capacity %d", palette_capacity);
  PR_REQUIRE(offsets[0] >= 0, "pr_png_parse: offsets_host[0] = %lld", (long long)offsets[0]);
  for (int f = 0; f < F; ++f)
    PR_REQUIRE(offsets[f + 1] >= offsets[f], "pr_png_parse: offsets_host[%d] = %lld is below offsets_host[%d] = %lld", f + 1,
               (long long)offsets[f + 1], f, (long long)offsets[f]);
  Out o;
  o.idat = idat;
  o.idat_cap = idat_capacity;
  o.palettes = palettes;
  o.pal_cap = palette_capacity;
  for (int f = 0; f < F; ++f) {
    const int idat_before = o.n_idat, pal_before = o.n_pal;
    const int st = parse_one(data, offsets[f], offsets[f + 1], &H, &W, &frames[f], &o);
    parse_status[f] = st;
    if (st != PR_PNG_OK) {
      memset(&frames[f], 0, sizeof frames[f]);   // bpp = 0: the device zero-fills this frame
      frames[f].palette = -1;
      frames[f].first_idat = o.n_idat = idat_before;
      o.n_pal = pal_before;
      set_error("pr_png_parse: frame %d refused: %s", f, pr_png_refusal_name(st));
    }
  }
  counts[0] = o.n_idat;
  counts[1] = o.n_pal;
  counts[2] = H;
  counts[3] = W;
  if (o.n_idat > idat_capacity || o.n_pal > palette_capacity) {
    set_error("pr_png_parse: %d IDAT ranges and %d palettes are needed, room for %d and %d was given", o.n_idat, o.n_pal,
              idat_capacity, palette_capacity);
    return PR_ERR_CAPACITY;
  }
  return PR_OK;
}
