// Stand-alone host driver of the PNG encoder for tests/test_png_encode_native.py: csrc/png_enc_host.cc (plan, bound, workspace)
// and the one-lane instantiation of csrc/png_enc_device.h (filters, adaptive choice, tokens, code construction, bits, stored
// fallback, checksum algebra), built by g++ under ASan + UBSan.  Every frame is handled on its own and every
// buffer -- the pixels, the row filters, each segment's staging area (5 + n bytes: the contract's bound), the file (exactly
// pr_png_encode_bound) -- is a heap block of EXACTLY its size, so that one byte read or written outside shows.
//
//   png_enc_native each <pack.bin> <out.bin>
// pack.bin: int32 n, then per frame int32 H, W, filter, mode, bgr and H * W * 3 pixels.  out.bin, per frame: int32 size, the file.
//   png_enc_native errors
// prints "ok" when every bad argument of the plan, bound and workspace functions is refused.
#define NATIVE_QUIET_ERRORS    // `errors` provokes every refusal and reads its message
#include "native_common.h"
#include "png_enc_host.cc"
using pr::g_error;

using namespace pr::pngenc;

static std::vector<uint8_t> encode_one(const uint8_t* px, int H, int W, int filter, int mode, int bgr) {
  pr_png_enc_plan plan;
  if (pr_png_encode_plan(filter, mode, H, W, &plan) != PR_OK) {
    fprintf(stderr, "plan refused: %s\n", g_error);
    exit(3);
  }
  const EncLane1 p;
  const int64_t raw = plan.raw_bytes;
  const int nseg = plan.n_segments;
  std::unique_ptr<uint8_t[]> rowf(new uint8_t[(size_t)H]);
  FilterSrc src{px, H, W, bgr, mode == PR_PNG_ENC_STORED ? 0 : filter, rowf.get()};
  if (src.fixed == PR_PNG_ENC_FILTER_ADAPTIVE)
    for (int r = 0; r < H; ++r) rowf[r] = (uint8_t)choose_row(p, src, r);
  std::unique_ptr<SegScratch<1>> scratch(new SegScratch<1>);
  std::vector<std::unique_ptr<uint8_t[]>> stage((size_t)nseg);
  std::vector<SegRec> rec((size_t)nseg);
  uint64_t coded = 0;
  for (int s = 0; s < nseg; ++s) {
    const int64_t begin = (int64_t)s * kSeg;
    const int n = (int)(raw - begin < kSeg ? raw - begin : kSeg);
    stage[s].reset(new uint8_t[(size_t)n + 5]);
    encode_segment(p, *scratch, src, begin, n, s == nseg - 1, mode, plan.crc_pow, stage[s].get(), &rec[s]);
    if (rec[s].len > (uint32_t)n + 5) {
      fprintf(stderr, "segment %d reports %u bytes, above 5 + %d\n", s, rec[s].len, n);
      exit(3);
    }
    coded += rec[s].len;
  }
  FrameSums sums;
  uint64_t at = 0;
  for (int s = 0; s < nseg; ++s) {
    at += rec[s].len;
    const int64_t end = (int64_t)(s + 1) * kSeg < raw ? (int64_t)(s + 1) * kSeg : raw;
    add_segment(sums, rec[s], coded - at, (uint64_t)(raw - end), plan.crc_pow);
  }
  const uint32_t adler = frame_adler(sums, (uint64_t)raw);
  const uint32_t crc = frame_idat_crc(sums, plan.idat_crc_head, coded, adler, plan.crc_pow);
  const size_t size = PR_PNG_ENC_HEAD_BYTES + coded + 8 + PR_PNG_ENC_TAIL_BYTES, bound = pr_png_encode_bound(H, W);
  if (size > bound) {
    fprintf(stderr, "a file of %zu bytes exceeds the bound %zu\n", size, bound);
    exit(3);
  }
  std::unique_ptr<uint8_t[]> file(new uint8_t[bound]);
  uint8_t* o = file.get();
  memcpy(o, plan.head, PR_PNG_ENC_HEAD_BYTES);
  const uint32_t idat_len = (uint32_t)(2 + coded + 4);
  for (int k = 0; k < 4; ++k) o[33 + k] = (uint8_t)(idat_len >> (24 - 8 * k));
  o += PR_PNG_ENC_HEAD_BYTES;
  for (int s = 0; s < nseg; ++s) memcpy(o, stage[s].get(), rec[s].len), o += rec[s].len;
  for (int k = 0; k < 4; ++k) *o++ = (uint8_t)(adler >> (24 - 8 * k));
  for (int k = 0; k < 4; ++k) *o++ = (uint8_t)(crc >> (24 - 8 * k));
  memcpy(o, plan.tail, PR_PNG_ENC_TAIL_BYTES);
  return std::vector<uint8_t>(file.get(), file.get() + size);
}

static int check_errors() {
  pr_png_enc_plan plan;
  int bad = 0;
  auto refused = [&](int rc, const char* word) {
    if (rc != PR_ERR_INVALID || !strstr(g_error, word)) ++bad, fprintf(stderr, "rc %d, message '%s', wanted '%s'\n", rc, g_error, word);
    g_error[0] = 0;
  };
  refused(pr_png_encode_plan(5, 1, 4, 4, nullptr), "null plan");
  refused(pr_png_encode_plan(6, 1, 4, 4, &plan), "filter");
  refused(pr_png_encode_plan(-1, 1, 4, 4, &plan), "filter");
  refused(pr_png_encode_plan(5, 2, 4, 4, &plan), "mode");
  refused(pr_png_encode_plan(5, 1, 0, 4, &plan), "size");
  refused(pr_png_encode_plan(5, 1, 4, PR_PNG_MAX_SIDE + 1, &plan), "size");
  if (pr_png_encode_plan(5, 1, PR_PNG_MAX_SIDE, PR_PNG_MAX_SIDE, &plan) != PR_OK) ++bad;
  if (pr_png_encode_bound(0, 4) || pr_png_encode_bound(4, 4097) || pr_png_encode_bound(1, 1) != 72) ++bad;
  if (pr_png_encode_workspace_bytes(0, 4, 4) || pr_png_encode_workspace_bytes(70000, 4, 4) || pr_png_encode_workspace_bytes(1, 0, 4) ||
      pr_png_encode_workspace_bytes(2, 9, 683) < 2 * 2 * (size_t)kStage)
    ++bad;
  puts(bad ? "failed" : "ok");
  return bad ? 1 : 0;
}

int main(int argc, char** argv) {
  if (argc == 2 && !strcmp(argv[1], "errors")) return check_errors();
  if (argc != 4 || strcmp(argv[1], "each") != 0) {
    fprintf(stderr, "usage: png_enc_native each <pack.bin> <out.bin> | errors\n");
    return 2;
  }
  std::ifstream f(argv[2], std::ios::binary);
  const std::vector<uint8_t> pack((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
  std::ofstream out(argv[3], std::ios::binary);
  int32_t n = 0;
  memcpy(&n, pack.data(), 4);
  size_t at = 4;
  for (int i = 0; i < n; ++i) {
    int32_t h[5];
    memcpy(h, pack.data() + at, sizeof h);
    at += sizeof h;
    const size_t npx = (size_t)h[0] * h[1] * 3;
    std::unique_ptr<uint8_t[]> px(new uint8_t[npx]);
    memcpy(px.get(), pack.data() + at, npx);
    at += npx;
    const std::vector<uint8_t> file = encode_one(px.get(), h[0], h[1], h[2], h[3], h[4]);
    const int32_t size = (int32_t)file.size();
    out.write((const char*)&size, 4);
    out.write((const char*)file.data(), size);
  }
  return 0;
}
