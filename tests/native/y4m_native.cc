// csrc/y4m_host.cc and csrc/yuv.hip on the host (see host_shim.h), built by tests/test_y4m_native.py with
// g++ under ASan + UBSan.
//   y4m_native frames <in> <out>   a whole YUV4MPEG2 stream through pr_y4m_parse_header, pr_y4m_index, pr_yuv_plan and
//       pr_yuv_frames (with h, w > 0 also pr_resize_plan: the fused downscale), every buffer an exact-size heap block, once per
//       alignment 0..3 of the output's first byte (the block is then that much larger and the bytes in front of the output must
//       keep their fill; behind it the block ends).  in: int32 matrix, full_range (-1: the header's), bgr, h, w, n; u8 stream[n].
//       out: int32 F, H, W, chroma, full_range of the header, fps_num, fps_den, header_bytes, h, w, mode, the six plan integers,
//       int64 offsets[F] (in the stream), then four times u8 dst[F,h,w,3].
//   y4m_native refusals   every argument error of the entries returns PR_ERR_INVALID (the words go to stderr).
#include "common.h"
#include "native_common.h"

#include "resize_host.cc"
#include "y4m_host.cc"
#include "yuv.hip"

static int run_frames(const char* in, const char* outp) {
  std::ifstream f(in, std::ios::binary);
  int32_t hd[6];
  f.read((char*)hd, sizeof hd);
  const int matrix = hd[0], bgr = hd[2], n = hd[5];
  int full = hd[1], h = hd[3], w = hd[4];
  auto data = exact<uint8_t>((size_t)n);
  f.read((char*)data.get(), n);
  if (!f) return 10;
  pr_y4m_info info;
  if (pr_y4m_parse_header(data.get(), n, &info) != PR_OK) return 11;
  const int max_frames = (int)((n - info.header_bytes) / (info.frame_bytes + 6)) + 1;
  auto offsets = exact<int64_t>((size_t)max_frames);
  int32_t F = -1;
  int64_t used = -1;
  if (pr_y4m_index(data.get() + info.header_bytes, n - info.header_bytes, &info, offsets.get(), max_frames, &F, &used) != PR_OK) return 12;
  if (used != n - info.header_bytes) return 13;
  for (int i = 0; i < F; ++i) offsets[i] += info.header_bytes;
  if (full < 0) full = info.full_range == 1;
  pr_yuv_args a;
  memset(&a, 0, sizeof a);
  if (pr_yuv_plan(matrix, full, &a.plan) != PR_OK) return 14;
  const int H = info.height, W = info.width;
  std::unique_ptr<int32_t[]> xofs, yofs;
  std::unique_ptr<int16_t[]> xcoef, ycoef;
  int32_t mode = 0;
  if (h > 0) {
    xofs = exact<int32_t>((size_t)w), yofs = exact<int32_t>((size_t)h);
    xcoef = exact<int16_t>((size_t)2 * w), ycoef = exact<int16_t>((size_t)2 * h);
    if (pr_resize_plan(H, W, h, w, xofs.get(), xcoef.get(), yofs.get(), ycoef.get(), &mode) != PR_OK) return 15;
    a.xofs = xofs.get(), a.xcoef = xcoef.get(), a.yofs = yofs.get(), a.ycoef = ycoef.get();
    a.h = h, a.w = w, a.mode = mode;
  }
  a.data = data.get(), a.data_bytes = n, a.offsets = offsets.get();
  a.F = F, a.H = H, a.W = W, a.chroma = info.chroma, a.bgr = bgr;
  const int oh = h > 0 ? h : H, ow = h > 0 ? w : W;
  const size_t dst_bytes = (size_t)F * oh * ow * 3;
  std::ofstream o(outp, std::ios::binary);
  const int32_t head[11] = {F, H, W, info.chroma, info.full_range, info.fps_num, info.fps_den, info.header_bytes, oh, ow, mode};
  o.write((const char*)head, sizeof head);
  o.write((const char*)&a.plan, sizeof a.plan);
  o.write((const char*)offsets.get(), 8 * (std::streamsize)F);
  for (int shift = 0; shift < 4; ++shift) {
    const size_t block = dst_bytes + shift;   // the output ends where the block ends
    auto dst = exact<uint8_t>(block);
    if ((uintptr_t)dst.get() & 3) return 16;
    memset(dst.get(), 0xAB, block);
    a.dst = dst.get() + shift;
    if (pr_yuv_frames(&a, nullptr) != PR_OK) return 17;
    for (size_t i = 0; i < (size_t)shift; ++i)
      if (dst[i] != 0xAB) {
        fprintf(stderr, "alignment %d: byte %zu in front of the output was written\n", shift, i);
        return 18;
      }
    o.write((char*)dst.get() + shift, (std::streamsize)dst_bytes);
  }
  // a payload that does not lie inside the chunk is written as zeros and none of it is read: frame 0's offset pushed
  // past the end, then in front of the start, the chunk still an exact block
  if (F > 0) {
    auto dst = exact<uint8_t>(dst_bytes);
    a.dst = dst.get();
    const int64_t keep = offsets[0];
    for (int64_t bad : {(int64_t)n - info.frame_bytes + 1, (int64_t)-1}) {
      offsets[0] = bad;
      memset(dst.get(), 0xAB, dst_bytes);
      if (pr_yuv_frames(&a, nullptr) != PR_OK) return 19;
      for (size_t i = 0; i < (size_t)oh * ow * 3; ++i)
        if (dst[i] != 0) return 20;
    }
    offsets[0] = keep;
  }
  return 0;
}

static int run_refusals() {
  const char stream[] = "YUV4MPEG2 W4 H4 F25:1\nFRAME\n";
  auto data = exact<uint8_t>(sizeof stream - 1 + 24);
  memcpy(data.get(), stream, sizeof stream - 1);
  const int64_t n = (int64_t)sizeof stream - 1 + 24;
  pr_y4m_info info, untouched;
  memset(&info, 0x5A, sizeof info);
  untouched = info;
  int bad = 0, count = 0;
  auto refused = [&](int rc) { ++count, bad += rc != PR_ERR_INVALID; };
  refused(pr_y4m_parse_header(nullptr, n, &info));
  refused(pr_y4m_parse_header(data.get(), n, nullptr));
  refused(pr_y4m_parse_header(data.get(), -1, &info));
  if (memcmp(&info, &untouched, sizeof info)) return 30;      // a refused call writes nothing
  if (pr_y4m_parse_header(data.get(), n, &info) != PR_OK || info.frame_bytes != 24 || info.header_bytes != 22) return 31;
  int64_t offsets[2] = {-5, -5}, used = -5;
  int32_t F = -5;
  const uint8_t* body = data.get() + info.header_bytes;
  const int64_t m = n - info.header_bytes;
  refused(pr_y4m_index(nullptr, m, &info, offsets, 2, &F, &used));
  refused(pr_y4m_index(body, m, nullptr, offsets, 2, &F, &used));
  refused(pr_y4m_index(body, m, &info, nullptr, 2, &F, &used));
  refused(pr_y4m_index(body, m, &info, offsets, 2, nullptr, &used));
  refused(pr_y4m_index(body, m, &info, offsets, 2, &F, nullptr));
  refused(pr_y4m_index(body, -1, &info, offsets, 2, &F, &used));
  refused(pr_y4m_index(body, m, &info, offsets, -1, &F, &used));
  pr_y4m_info wrong = info;
  wrong.frame_bytes = 23;
  refused(pr_y4m_index(body, m, &wrong, offsets, 2, &F, &used));
  wrong = info, wrong.chroma = 5;
  refused(pr_y4m_index(body, m, &wrong, offsets, 2, &F, &used));
  if (offsets[0] != -5 || F != -5 || used != -5) return 32;
  if (pr_y4m_index(body, m, &info, offsets, 2, &F, &used) != PR_OK || F != 1 || used != m || offsets[0] != 6) return 33;
  pr_yuv_coeffs plan;
  memset(&plan, 0x5A, sizeof plan);
  const pr_yuv_coeffs plan0 = plan;
  refused(pr_yuv_plan(2, 0, &plan));
  refused(pr_yuv_plan(-1, 0, &plan));
  refused(pr_yuv_plan(0, 2, &plan));
  refused(pr_yuv_plan(0, 0, nullptr));
  if (memcmp(&plan, &plan0, sizeof plan)) return 34;
  if (pr_yuv_plan(PR_YUV_601, 0, &plan) != PR_OK || plan.cy != 76309 || plan.crv != 104597 || plan.cbu != 132201 || plan.cgu != 25675 ||
      plan.cgv != 53279 || plan.yo != 16)
    return 35;

  auto xofs = exact<int32_t>(2), yofs = exact<int32_t>(2);
  auto xcoef = exact<int16_t>(4), ycoef = exact<int16_t>(4);
  int32_t mode = -1;
  if (pr_resize_plan(4, 4, 2, 2, xofs.get(), xcoef.get(), yofs.get(), ycoef.get(), &mode) != PR_OK || mode != PR_RESIZE_HALF) return 36;
  auto dst = exact<uint8_t>(4 * 4 * 3);
  memset(dst.get(), 0xAB, 4 * 4 * 3);
  int64_t off = info.header_bytes + 6;
  pr_yuv_args good;
  memset(&good, 0, sizeof good);
  good.data = data.get(), good.data_bytes = n, good.offsets = &off, good.dst = dst.get(), good.plan = plan;
  good.F = 1, good.H = 4, good.W = 4, good.chroma = PR_Y4M_C420JPEG;
  pr_yuv_args a;
  refused(pr_yuv_frames(nullptr, nullptr));
  a = good, a.F = -1;
  refused(pr_yuv_frames(&a, nullptr));
  a = good, a.H = 0;
  refused(pr_yuv_frames(&a, nullptr));
  a = good, a.W = 4097;
  refused(pr_yuv_frames(&a, nullptr));
  a = good, a.chroma = 5;
  refused(pr_yuv_frames(&a, nullptr));
  a = good, a.chroma = -1;
  refused(pr_yuv_frames(&a, nullptr));
  a = good, a.data_bytes = -1;
  refused(pr_yuv_frames(&a, nullptr));
  a = good, a.data = nullptr;
  refused(pr_yuv_frames(&a, nullptr));
  a = good, a.offsets = nullptr;
  refused(pr_yuv_frames(&a, nullptr));
  a = good, a.dst = nullptr;
  refused(pr_yuv_frames(&a, nullptr));
  pr_yuv_args half = good;
  half.h = 2, half.w = 2, half.mode = mode;
  half.xofs = xofs.get(), half.xcoef = xcoef.get(), half.yofs = yofs.get(), half.ycoef = ycoef.get();
  a = half, a.h = 0;
  refused(pr_yuv_frames(&a, nullptr));
  a = half, a.w = 4097;
  refused(pr_yuv_frames(&a, nullptr));
  a = half, a.mode = PR_RESIZE_LINEAR;
  refused(pr_yuv_frames(&a, nullptr));
  a = half, a.xofs = nullptr;
  refused(pr_yuv_frames(&a, nullptr));
  a = half, a.xcoef = nullptr;
  refused(pr_yuv_frames(&a, nullptr));
  a = half, a.yofs = nullptr;
  refused(pr_yuv_frames(&a, nullptr));
  a = half, a.ycoef = nullptr;
  refused(pr_yuv_frames(&a, nullptr));
  a = good, a.xofs = xofs.get();                                   // only some of the downscale's arguments
  refused(pr_yuv_frames(&a, nullptr));
  a = good, a.mode = PR_RESIZE_HALF;
  refused(pr_yuv_frames(&a, nullptr));
  for (int i = 0; i < 4 * 4 * 3; ++i)
    if (dst[i] != 0xAB) return 37;                                  // no refused call did device work
  a = good, a.F = 0, a.data = nullptr, a.dst = nullptr, a.H = -3;   // F = 0 is legal whatever else is given
  if (pr_yuv_frames(&a, nullptr) != PR_OK) return 38;
  if (pr_yuv_frames(&good, nullptr) != PR_OK || pr_yuv_frames(&half, nullptr) != PR_OK) return 39;
  printf("y4m_native: %d of %d bad calls refused\n", count - bad, count);
  return bad ? 40 : 0;
}

int main(int argc, char** argv) {
  if (argc >= 4 && !strcmp(argv[1], "frames")) return run_frames(argv[2], argv[3]);
  if (argc >= 2 && !strcmp(argv[1], "refusals")) return run_refusals();
  return 2;
}
