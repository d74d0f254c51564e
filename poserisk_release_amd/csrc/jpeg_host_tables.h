// What the two marker parsers (csrc/jpeg_host.cc: pr_jpeg_parse; csrc/jpeg_scans_host.cc: pr_jpeg_parse_scans) share: the
// bounded reader, a Huffman table as a file defines it, the device's decode table built from it and the comparison that stores
// identical table sets once.  Device-free; included after host_common.h.
#pragma once
#include <cstring>

namespace pr {
namespace {

const unsigned char kZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                   41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                   30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

struct Reader {
  const uint8_t* p;
  int64_t pos, end;
  bool ok(int64_t n) const { return n >= 0 && end - pos >= n; }
  int u8() { return p[pos++]; }
  int u16() {
    const int v = p[pos] << 8 | p[pos + 1];
    pos += 2;
    return v;
  }
};

struct RawHuff {
  bool defined = false;
  uint8_t bits[17] = {};
  uint8_t vals[256] = {};
};

// bits / vals -> the device's decode table; false when the counts do not form a prefix code
bool build_table(const RawHuff& r, pr_jpeg_hufftab* t) {
  memset(t, 0, sizeof *t);
  int total = 0;
  for (int l = 1; l <= 16; ++l) total += r.bits[l];
  if (total > 256) return false;
  int code = 0, k = 0;
  for (int l = 1; l <= 16; ++l) {
    t->valoff[l] = k - code;
    if (r.bits[l]) {
      if (code + r.bits[l] > (1 << l)) return false;
      for (int i = 0; i < r.bits[l]; ++i, ++code, ++k)
        if (l <= PR_JPEG_LOOK_BITS) {
          const int lo = code << (PR_JPEG_LOOK_BITS - l), n = 1 << (PR_JPEG_LOOK_BITS - l);
          for (int j = 0; j < n; ++j) t->look[lo + j] = (uint16_t)(l << 8 | r.vals[k]);
        }
      t->maxcode[l] = code - 1;
    } else {
      t->maxcode[l] = -1;
    }
    code <<= 1;
  }
  memcpy(t->vals, r.vals, 256);
  t->defined = 1;
  return true;
}

uint64_t fnv(const void* p, size_t n) {
  uint64_t h = 1469598103934665603ull;
  for (size_t i = 0; i < n; ++i) h = (h ^ ((const uint8_t*)p)[i]) * 1099511628211ull;
  return h;
}

bool same_raw(const RawHuff* a, const RawHuff* b) {
  for (int i = 0; i < 4; ++i) {
    if (a[i].defined != b[i].defined) return false;
    if (a[i].defined && (memcmp(a[i].bits, b[i].bits, 17) || memcmp(a[i].vals, b[i].vals, 256))) return false;
  }
  return true;
}

}  // namespace
}  // namespace pr
