// csrc/resize_host.cc and csrc/resize.hip on the host (see host_shim.h), built by tests/test_frontend_native.py with
// g++ under ASan + UBSan.
//   resize_native resize <in> <out>   F frames through pr_resize_plan and pr_resize_frames, every buffer an exact-size heap
//       block, once per alignment 0..3 of the output's first byte (the block is then that much larger and the bytes in front of
//       the output must keep their fill; behind it the block ends).  in: int32 F, H, W, h, w; u8 frames[F,H,W,3].   out: int32 mode, int32 xofs[w],
//       int16 xcoef[2w], int32 yofs[h], int16 ycoef[2h], then four times u8 dst[F,h,w,3].
//   resize_native refusals   every argument error of the two entries returns PR_ERR_INVALID (the words go to stderr).
#include "common.h"
#include "native_common.h"

#include "resize_host.cc"
#include "resize.hip"

static int run_resize(const char* in, const char* outp) {
  std::ifstream f(in, std::ios::binary);
  int32_t hd[5];
  f.read((char*)hd, sizeof hd);
  const int F = hd[0], H = hd[1], W = hd[2], h = hd[3], w = hd[4];
  const size_t src_bytes = (size_t)F * H * W * 3, dst_bytes = (size_t)F * h * w * 3;
  auto src = exact<uint8_t>(src_bytes);
  f.read((char*)src.get(), (std::streamsize)src_bytes);
  if (!f) return 10;
  auto xofs = exact<int32_t>((size_t)w), yofs = exact<int32_t>((size_t)h);
  auto xcoef = exact<int16_t>((size_t)2 * w), ycoef = exact<int16_t>((size_t)2 * h);
  int32_t mode = -1;
  if (pr_resize_plan(H, W, h, w, xofs.get(), xcoef.get(), yofs.get(), ycoef.get(), &mode) != PR_OK) return 11;
  std::ofstream o(outp, std::ios::binary);
  o.write((char*)&mode, 4);
  o.write((char*)xofs.get(), 4 * w);
  o.write((char*)xcoef.get(), 4 * w);
  o.write((char*)yofs.get(), 4 * h);
  o.write((char*)ycoef.get(), 4 * h);
  for (int shift = 0; shift < 4; ++shift) {
    // operator new[] returns 16-byte aligned blocks: dst = block + shift starts at alignment `shift`, and with frames of a
    // size that is no multiple of 4 the later frames start at the other alignments too
    const size_t block = dst_bytes + shift;   // the output ends where the block ends
    auto dst = exact<uint8_t>(block);
    if ((uintptr_t)dst.get() & 3) return 12;
    memset(dst.get(), 0xAB, block);
    if (pr_resize_frames(src.get(), F, H, W, dst.get() + shift, h, w, xofs.get(), xcoef.get(), yofs.get(), ycoef.get(), mode,
                         nullptr) != PR_OK)
      return 13;
    for (size_t i = 0; i < block; ++i)
      if ((i < (size_t)shift || i >= shift + dst_bytes) && dst[i] != 0xAB) {
        fprintf(stderr, "alignment %d: byte %zu outside the output was written\n", shift, i);
        return 14;
      }
    o.write((char*)dst.get() + shift, (std::streamsize)dst_bytes);
  }
  return 0;
}

static int run_refusals() {
  auto xofs = exact<int32_t>(8), yofs = exact<int32_t>(8);
  auto xcoef = exact<int16_t>(16), ycoef = exact<int16_t>(16);
  auto src = exact<uint8_t>(16 * 16 * 3), dst = exact<uint8_t>(8 * 8 * 3);
  int32_t mode = -1;
  int32_t *xo = xofs.get(), *yo = yofs.get();
  int16_t *xc = xcoef.get(), *yc = ycoef.get();
  int bad = 0, n = 0;
  auto refused = [&](int rc) { ++n, bad += rc != PR_ERR_INVALID; };
  refused(pr_resize_plan(0, 16, 8, 8, xo, xc, yo, yc, &mode));
  refused(pr_resize_plan(16, 4097, 8, 8, xo, xc, yo, yc, &mode));
  refused(pr_resize_plan(16, 16, 0, 8, xo, xc, yo, yc, &mode));
  refused(pr_resize_plan(16, 16, 8, 4097, xo, xc, yo, yc, &mode));
  refused(pr_resize_plan(16, 16, 8, 8, nullptr, xc, yo, yc, &mode));
  refused(pr_resize_plan(16, 16, 8, 8, xo, nullptr, yo, yc, &mode));
  refused(pr_resize_plan(16, 16, 8, 8, xo, xc, nullptr, yc, &mode));
  refused(pr_resize_plan(16, 16, 8, 8, xo, xc, yo, nullptr, &mode));
  refused(pr_resize_plan(16, 16, 8, 8, xo, xc, yo, yc, nullptr));
  if (mode != -1) return 20;                       // a refused call writes nothing
  if (pr_resize_plan(16, 16, 8, 8, xo, xc, yo, yc, &mode) != PR_OK || mode != PR_RESIZE_HALF) return 21;
  refused(pr_resize_frames(src.get(), -1, 16, 16, dst.get(), 8, 8, xo, xc, yo, yc, mode, nullptr));
  refused(pr_resize_frames(src.get(), 1, 16, 5000, dst.get(), 8, 8, xo, xc, yo, yc, mode, nullptr));
  refused(pr_resize_frames(src.get(), 1, 16, 16, dst.get(), 8, 8, xo, xc, yo, yc, PR_RESIZE_LINEAR, nullptr));
  refused(pr_resize_frames(nullptr, 1, 16, 16, dst.get(), 8, 8, xo, xc, yo, yc, mode, nullptr));
  refused(pr_resize_frames(src.get(), 1, 16, 16, nullptr, 8, 8, xo, xc, yo, yc, mode, nullptr));
  refused(pr_resize_frames(src.get(), 1, 16, 16, dst.get(), 8, 8, nullptr, xc, yo, yc, mode, nullptr));
  refused(pr_resize_frames(src.get(), 1, 16, 16, dst.get(), 8, 8, xo, nullptr, yo, yc, mode, nullptr));
  refused(pr_resize_frames(src.get(), 1, 16, 16, dst.get(), 8, 8, xo, xc, nullptr, yc, mode, nullptr));
  refused(pr_resize_frames(src.get(), 1, 16, 16, dst.get(), 8, 8, xo, xc, yo, nullptr, mode, nullptr));
  if (pr_resize_frames(nullptr, 0, 16, 16, nullptr, 8, 8, nullptr, nullptr, nullptr, nullptr, 7, nullptr) != PR_OK) return 22;
  printf("resize_native: %d of %d bad calls refused\n", n - bad, n);
  return bad ? 23 : 0;
}

int main(int argc, char** argv) {
  if (argc >= 4 && !strcmp(argv[1], "resize")) return run_resize(argv[2], argv[3]);
  if (argc >= 2 && !strcmp(argv[1], "refusals")) return run_refusals();
  return 2;
}
