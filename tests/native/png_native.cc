// Stand-alone host driver of the PNG decoder for tests/test_png_native.py: csrc/png_host.cc (the chunk walk) and the one-lane
// instantiation of csrc/png_device.h (bit reader, tables, symbol decode, every validation decision, Adler-32, unfilter), built by
// g++ under ASan + UBSan.  Every file is handled on its own and every buffer -- the file, the gathered stream,
// the inflated scanlines, the pixels -- is a heap block of EXACTLY its size, so that one byte read or written outside shows.
//
//   png_native each <pack.bin> <out.bin> <bgr>
// pack.bin: int64 n, int64 offsets[n + 1], the files back to back.  out.bin, per file: int32 head[8] = parse_status, IDAT
// ranges, palettes, H, W, status, 0, 0; for an accepted file then its pr_png_frame, its ranges (relative to the file) and
// H * W * 3 pixels.
#define NATIVE_QUIET_ERRORS    // thousands of damaged streams: the refusals' words are not what is checked
#include "native_common.h"
#include "png_device.h"
#include "png_host.cc"

using namespace pr::png;

// What pr_png_decode's three kernels do for one frame, on the host: -> status, pixels (H * W * 3)
static int decode_one(const uint8_t* file, int64_t n, const pr_png_frame& fr, const pr_png_idat* idat, const uint8_t* palettes, int bgr,
                      uint8_t* pixels) {
  const PngLane1 p;
  const int H = fr.height, W = fr.width;
  // as on the device, the stream keeps its first range's phase: it starts `skew` bytes into its block, behind filler
  const int64_t skew = idat[fr.first_idat].begin & 15;
  std::unique_ptr<uint8_t[]> zblock(new uint8_t[(size_t)(skew + fr.zlib_bytes)]);
  memset(zblock.get(), 0xA5, (size_t)skew);
  uint8_t* const zs = zblock.get() + skew;
  int64_t at = 0;
  for (int i = 0; i < fr.n_idat; ++i) {
    const pr_png_idat& g = idat[fr.first_idat + i];
    if (g.begin < 0 || g.begin > g.end || g.end > n || at + (g.end - g.begin) > fr.zlib_bytes) {
      fprintf(stderr, "range %d of the parser lies outside its file\n", i);
      exit(3);
    }
    memcpy(zs + at, file + g.begin, (size_t)(g.end - g.begin));
    at += g.end - g.begin;
  }
  if (at != fr.zlib_bytes) {
    fprintf(stderr, "the parser's ranges hold %lld bytes, its frame says %lld\n", (long long)at, (long long)fr.zlib_bytes);
    exit(3);
  }
  const int64_t stride = 1 + (int64_t)W * fr.bpp, nraw = stride * H;
  std::unique_ptr<uint8_t[]> raw(new uint8_t[(size_t)nraw]);
  std::unique_ptr<Tables> dyn(new Tables), fixed(new Tables);
  build_fixed(p, fixed.get());
  uint32_t adler = 0;
  int st = inflate(p, zblock.get(), skew, fr.zlib_bytes, raw.get(), nraw, dyn.get(), fixed.get(), &adler, (InflateStats*)nullptr);
  if (st) {
    memset(pixels, 0, (size_t)H * W * 3);
    return st;
  }
  uint32_t s1 = 0, s2 = 0;
  adler_partial(raw.get(), nraw, 0, 1, &s1, &s2);
  if (adler_combine(s1, s2, nraw) != adler) st |= PR_PNG_ST_CHECKSUM;
  for (int r = 0; r < H; ++r)
    if (unfilter_pass(p, raw.get(), H, W, fr.bpp, r)) st |= PR_PNG_ST_FILTER;
  const uint8_t* pal = fr.color_type == 3 ? palettes + (size_t)fr.palette * 768 : nullptr;
  for (int y = 0; y < H; ++y)
    for (int x = 0; x < W; ++x)
      colour_pixel(fr.color_type, fr.bpp, raw.get() + y * stride + 1 + (int64_t)x * fr.bpp, pal, bgr, pixels + ((size_t)y * W + x) * 3);
  return st;
}

int main(int argc, char** argv) {
  if (argc != 5 || strcmp(argv[1], "each") != 0) {
    fprintf(stderr, "usage: png_native each <pack.bin> <out.bin> <bgr>\n");
    return 2;
  }
  const Pack pack = read_pack(argv[2]);
  const int bgr = atoi(argv[4]);
  std::ofstream out(argv[3], std::ios::binary);
  for (int64_t s = 0; s < pack.F; ++s) {
    const int64_t len = pack.size(s);
    auto file = pack.copy(s);   // exact size: ASan sees the first byte outside
    const int64_t offsets[2] = {0, len};
    pr_png_frame fr;
    int32_t pst = 0, counts[4] = {0, 0, 0, 0};
    std::vector<pr_png_idat> idat(4);
    std::vector<uint8_t> pal(768);
    int rc = pr_png_parse(file.get(), offsets, 1, 0, 0, &fr, idat.data(), (int)idat.size(), pal.data(), 1, &pst, counts);
    if (rc == PR_ERR_CAPACITY) {
      idat.resize((size_t)counts[0]);
      rc = pr_png_parse(file.get(), offsets, 1, 0, 0, &fr, idat.data(), (int)idat.size(), pal.data(), 1, &pst, counts);
    }
    if (rc != PR_OK) {
      fprintf(stderr, "pr_png_parse returned %d on file %lld\n", rc, (long long)s);
      return 3;
    }
    int32_t head[8] = {pst, counts[0], counts[1], counts[2], counts[3], 0, 0, 0};
    if (pst != PR_PNG_OK) {
      out.write((const char*)head, sizeof head);
      continue;
    }
    std::unique_ptr<uint8_t[]> pixels(new uint8_t[(size_t)fr.height * fr.width * 3]);
    head[5] = decode_one(file.get(), len, fr, idat.data(), pal.data(), bgr, pixels.get());
    out.write((const char*)head, sizeof head);
    out.write((const char*)&fr, sizeof fr);
    out.write((const char*)idat.data(), (std::streamsize)(sizeof(pr_png_idat) * (size_t)counts[0]));
    out.write((const char*)pixels.get(), (std::streamsize)((size_t)fr.height * fr.width * 3));
  }
  return 0;
}
