// Host half of the YUV4MPEG2 reader (include/poserisk_hip.h, section j6): the stream header, the walk over the FRAME headers
// of a chunk, and the colour matrix's integers; and of the writer (section j7): the forward matrix's integers.  No device call
// and no HIP header: tests/test_y4m_native.py and tests/test_y4m_write_native.py build this file with g++ under sanitizers.
// Every refusal is decided before an output is written.
#include <algorithm>
#include <cmath>
#include <initializer_list>

#include "host_common.h"

namespace pr {
namespace {

const char* const kY4mRefusal[PR_Y4M_E_COUNT] = {
    "ok",
    "not a YUV4MPEG2 stream (no YUV4MPEG2 signature)",
    "the stream header does not end within 1024 bytes",
    "a malformed header field",
    "the header has no W or no H field",
    "a side outside 1..4096",
    "interlaced frames are not supported",
    "420paldv chroma siting is not supported",
    "samples of more than 8 bits are not supported",
    "4:1:1 chroma is not supported",
    "444alpha (an alpha plane) is not supported",
    "an unknown chroma layout",
    "no FRAME header where a frame must begin",
};

bool starts_with(const uint8_t* p, int64_t n, const char* word) {
  const int64_t len = (int64_t)strlen(word);
  return n >= len && memcmp(p, word, (size_t)len) == 0;
}

// a decimal number of 1..9 digits filling [p, e) exactly; -1 otherwise
long number(const uint8_t* p, const uint8_t* e) {
  if (p == e || e - p > 9) return -1;
  long v = 0;
  for (; p < e; ++p) {
    if (*p < '0' || *p > '9') return -1;
    v = v * 10 + (*p - '0');
  }
  return v;
}

bool is_word(const uint8_t* p, const uint8_t* e, const char* word) {
  return (size_t)(e - p) == strlen(word) && memcmp(p, word, (size_t)(e - p)) == 0;
}

// The C field's value -> a layout, or a refusal.
int chroma_of(const uint8_t* p, const uint8_t* e, int32_t* chroma) {
  if (is_word(p, e, "420jpeg") || is_word(p, e, "420")) return *chroma = PR_Y4M_C420JPEG, PR_Y4M_OK;
  if (is_word(p, e, "420mpeg2")) return *chroma = PR_Y4M_C420MPEG2, PR_Y4M_OK;
  if (is_word(p, e, "422")) return *chroma = PR_Y4M_C422, PR_Y4M_OK;
  if (is_word(p, e, "444")) return *chroma = PR_Y4M_C444, PR_Y4M_OK;
  if (is_word(p, e, "mono")) return *chroma = PR_Y4M_CMONO, PR_Y4M_OK;
  if (is_word(p, e, "420paldv")) return PR_Y4M_E_PALDV;
  if (is_word(p, e, "444alpha")) return PR_Y4M_E_ALPHA;
  if (is_word(p, e, "411")) return PR_Y4M_E_411;
  // 420p10, 422p12, 444p16, mono10, ...: a known base, then an optional 'p', then digits only
  for (const char* base : {"420", "422", "444", "mono"}) {
    const size_t len = strlen(base);
    if ((size_t)(e - p) > len && memcmp(p, base, len) == 0) {
      const uint8_t* q = p + len;
      if (*q == 'p') ++q;
      if (number(q, e) > 8) return PR_Y4M_E_HIGH_DEPTH;
    }
  }
  return PR_Y4M_E_CHROMA;
}

int refuse(const char* who, int code) {
  set_error("%s: %s", who, kY4mRefusal[code]);
  return code;
}

int64_t frame_payload_bytes(int W, int H, int chroma) {
  const int64_t cw = (chroma == PR_Y4M_C420JPEG || chroma == PR_Y4M_C420MPEG2 || chroma == PR_Y4M_C422) ? (W + 1) / 2 : W;
  const int64_t ch = (chroma == PR_Y4M_C420JPEG || chroma == PR_Y4M_C420MPEG2) ? (H + 1) / 2 : H;
  return (int64_t)W * H + (chroma == PR_Y4M_CMONO ? 0 : 2 * cw * ch);
}

}  // namespace
}  // namespace pr

extern "C" const char* pr_y4m_refusal_name(int code) {
  return code >= 0 && code < PR_Y4M_E_COUNT ? pr::kY4mRefusal[code] : "unknown refusal code";
}

extern "C" int pr_y4m_parse_header(const uint8_t* data, int64_t n, pr_y4m_info* info) {
  using namespace pr;
  static const char* const who = "pr_y4m_parse_header";
  PR_REQUIRE(data, "pr_y4m_parse_header: null data_host");
  PR_REQUIRE(info, "pr_y4m_parse_header: null info_host");
  PR_REQUIRE(n >= 0, "pr_y4m_parse_header: n = %lld", (long long)n);
  const int64_t magic = 9;
  if (memcmp(data, "YUV4MPEG2", (size_t)std::min<int64_t>(n, magic)) != 0) return refuse(who, PR_Y4M_E_MAGIC);
  const int64_t limit = std::min<int64_t>(n, PR_Y4M_MAX_HEADER);
  int64_t end = magic;
  while (end < limit && data[end] != '\n') ++end;
  if (end >= limit) return refuse(who, PR_Y4M_E_HEADER);        // also a buffer shorter than the signature
  if (end > magic && data[magic] != ' ') return refuse(who, PR_Y4M_E_MAGIC);
  pr_y4m_info o;
  memset(&o, 0, sizeof o);
  o.full_range = -1;
  o.chroma = PR_Y4M_C420JPEG;
  long W = -1, H = -1;
  const uint8_t* p = data + magic;
  const uint8_t* const stop = data + end;
  while (p < stop) {
    if (*p == ' ') {
      ++p;
      continue;
    }
    const uint8_t* e = p;
    while (e < stop && *e != ' ') ++e;
    const uint8_t tag = *p;
    const uint8_t* v = p + 1;
    if (tag == 'W' || tag == 'H') {
      const long s = number(v, e);
      if (s < 0) return refuse(who, PR_Y4M_E_FIELD);
      (tag == 'W' ? W : H) = s;
    } else if (tag == 'F') {
      const uint8_t* colon = v;
      while (colon < e && *colon != ':') ++colon;
      const long num = number(v, colon), den = colon < e ? number(colon + 1, e) : -1;
      if (num < 0 || den < 0 || (den == 0 && num != 0)) return refuse(who, PR_Y4M_E_FIELD);
      o.fps_num = (int32_t)num, o.fps_den = (int32_t)den;
    } else if (tag == 'I') {
      if (e - v != 1) return refuse(who, PR_Y4M_E_FIELD);
      if (*v == 't' || *v == 'b' || *v == 'm') return refuse(who, PR_Y4M_E_INTERLACED);
      if (*v != 'p' && *v != '?') return refuse(who, PR_Y4M_E_FIELD);
    } else if (tag == 'C') {
      const int st = chroma_of(v, e, &o.chroma);
      if (st != PR_Y4M_OK) return refuse(who, st);
    } else if (tag == 'X') {
      if (is_word(v, e, "COLORRANGE=FULL")) o.full_range = 1;
      if (is_word(v, e, "COLORRANGE=LIMITED")) o.full_range = 0;
    }                                                           // A and every other tag: ignored
    p = e;
  }
  if (W < 0 || H < 0) return refuse(who, PR_Y4M_E_NO_SIZE);
  if (W < 1 || W > PR_RESIZE_MAX_SIDE || H < 1 || H > PR_RESIZE_MAX_SIDE) return refuse(who, PR_Y4M_E_SIZE);
  if (o.fps_den == 0) o.fps_num = 0;
  o.width = (int32_t)W, o.height = (int32_t)H;
  o.header_bytes = (int32_t)(end + 1);
  o.frame_bytes = frame_payload_bytes((int)W, (int)H, o.chroma);
  *info = o;
  return PR_OK;
}

extern "C" int pr_y4m_index(const uint8_t* data, int64_t n, const pr_y4m_info* info, int64_t* offsets, int max_frames,
                            int32_t* n_frames, int64_t* consumed) {
  using namespace pr;
  PR_REQUIRE(data, "pr_y4m_index: null data_host");
  PR_REQUIRE(info, "pr_y4m_index: null info_host");
  PR_REQUIRE(offsets, "pr_y4m_index: null offsets_host");
  PR_REQUIRE(n_frames, "pr_y4m_index: null n_frames_host");
  PR_REQUIRE(consumed, "pr_y4m_index: null consumed_host");
  PR_REQUIRE(n >= 0, "pr_y4m_index: n = %lld", (long long)n);
  PR_REQUIRE(max_frames >= 0, "pr_y4m_index: max_frames = %d", max_frames);
  PR_REQUIRE(info->width >= 1 && info->width <= PR_RESIZE_MAX_SIDE && info->height >= 1 && info->height <= PR_RESIZE_MAX_SIDE &&
                 info->chroma >= PR_Y4M_C420JPEG && info->chroma <= PR_Y4M_CMONO &&
                 info->frame_bytes == frame_payload_bytes(info->width, info->height, info->chroma),
             "pr_y4m_index: info is not what pr_y4m_parse_header fills (%d x %d, chroma %d, %lld bytes a frame)", info->width,
             info->height, info->chroma, (long long)info->frame_bytes);
  // first pass: find the frames and any refusal; second: write
  for (int pass = 0; pass < 2; ++pass) {
    int64_t pos = 0;
    int count = 0;
    while (count < max_frames) {
      const int64_t left = n - pos;
      if (left <= 0) break;
      if (memcmp(data + pos, "FRAME", (size_t)std::min<int64_t>(left, 5)) != 0 ||
          (left > 5 && data[pos + 5] != ' ' && data[pos + 5] != '\n')) {
        set_error("pr_y4m_index: frame %d: %s", count, kY4mRefusal[PR_Y4M_E_FRAME]);
        return PR_Y4M_E_FRAME;
      }
      const int64_t limit = std::min<int64_t>(left, PR_Y4M_MAX_FRAME_HEADER);
      int64_t end = 5;
      while (end < limit && data[pos + end] != '\n') ++end;
      if (end >= limit) {
        if (left < PR_Y4M_MAX_FRAME_HEADER) break;             // the header may end in the bytes that follow
        set_error("pr_y4m_index: frame %d: %s (its header does not end within %d bytes)", count, kY4mRefusal[PR_Y4M_E_FRAME],
                  PR_Y4M_MAX_FRAME_HEADER);
        return PR_Y4M_E_FRAME;
      }
      const int64_t payload = pos + end + 1;
      if (n - payload < info->frame_bytes) break;
      if (pass) offsets[count] = payload;
      ++count;
      pos = payload + info->frame_bytes;
    }
    if (pass) {
      *n_frames = count;
      *consumed = pos;
    }
  }
  return PR_OK;
}

extern "C" int pr_yuv_plan(int matrix, int full_range, pr_yuv_coeffs* plan) {
  using namespace pr;
  PR_REQUIRE(matrix == PR_YUV_601 || matrix == PR_YUV_709, "pr_yuv_plan: matrix = %d (PR_YUV_601 = 0 or PR_YUV_709 = 1)", matrix);
  PR_REQUIRE(full_range == 0 || full_range == 1, "pr_yuv_plan: full_range = %d (0 or 1)", full_range);
  PR_REQUIRE(plan, "pr_yuv_plan: null plan_host");
  const double kr = matrix == PR_YUV_601 ? 0.299 : 0.2126, kb = matrix == PR_YUV_601 ? 0.114 : 0.0722, kg = 1.0 - kr - kb;
  const double sy = full_range ? 1.0 : 255.0 / 219.0, sc = full_range ? 1.0 : 255.0 / 224.0;
  plan->cy = (int32_t)std::nearbyint(sy * 65536.0);
  plan->crv = (int32_t)std::nearbyint(2.0 * (1.0 - kr) * sc * 65536.0);
  plan->cbu = (int32_t)std::nearbyint(2.0 * (1.0 - kb) * sc * 65536.0);
  plan->cgu = (int32_t)std::nearbyint(2.0 * kb * (1.0 - kb) / kg * sc * 65536.0);
  plan->cgv = (int32_t)std::nearbyint(2.0 * kr * (1.0 - kr) / kg * sc * 65536.0);
  plan->yo = full_range ? 0 : 16;
  return PR_OK;
}

// Section j7: the integers of the forward matrix.  The green luma weight and the green chroma weights are what is left of
// the rows' sums, so that a grey pixel has no chroma and white and black land on the range's ends exactly.
extern "C" int pr_yuv_enc_plan(int matrix, int full_range, pr_yuv_enc_coeffs* plan) {
  using namespace pr;
  PR_REQUIRE(matrix == PR_YUV_601 || matrix == PR_YUV_709, "pr_yuv_enc_plan: matrix = %d (PR_YUV_601 = 0 or PR_YUV_709 = 1)", matrix);
  PR_REQUIRE(full_range == 0 || full_range == 1, "pr_yuv_enc_plan: full_range = %d (0 or 1)", full_range);
  PR_REQUIRE(plan, "pr_yuv_enc_plan: null plan_host");
  const double kr = matrix == PR_YUV_601 ? 0.299 : 0.2126, kb = matrix == PR_YUV_601 ? 0.114 : 0.0722;
  const double sy = full_range ? 1.0 : 219.0 / 255.0, sc = full_range ? 1.0 : 224.0 / 255.0;
  const int32_t ky = (int32_t)std::nearbyint(sy * 65536.0);
  plan->kyr = (int32_t)std::nearbyint(kr * sy * 65536.0);
  plan->kyb = (int32_t)std::nearbyint(kb * sy * 65536.0);
  plan->kyg = ky - plan->kyr - plan->kyb;
  plan->kc = (int32_t)std::nearbyint(sc * 32768.0);
  plan->kur = (int32_t)std::nearbyint(kr / (2.0 * (1.0 - kb)) * sc * 65536.0);
  plan->kug = plan->kc - plan->kur;
  plan->kvb = (int32_t)std::nearbyint(kb / (2.0 * (1.0 - kr)) * sc * 65536.0);
  plan->kvg = plan->kc - plan->kvb;
  plan->yo = full_range ? 0 : 16;
  return PR_OK;
}
