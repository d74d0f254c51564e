// csrc/y4m_host.cc and csrc/yuv_enc.hip on the host (see host_shim.h), built by tests/test_y4m_write_native.py with
// g++ under ASan + UBSan.
//   yuv_enc_native encode <in> <out>   a list of calls through pr_yuv_enc_plan and pr_yuv_encode, every buffer an exact-size heap
//       block: src ends where its block ends and begins 0..3 bytes into it, dst likewise (the bytes in front of dst must keep
//       their fill).  All sixteen pairs of alignments run and must give the same bytes; the stream is then read back by
//       pr_y4m_index.  in: int32 count, then per call int32 matrix, full_range, bgr, chroma, F, H, W, out_H, out_W and
//       u8 src[F,H,W,3].  out: per call int32 total, the nine plan integers, then four times u8 dst[total] (dst at alignment
//       0, 1, 2, 3).
//   yuv_enc_native refusals   every argument error of the two entries returns PR_ERR_INVALID (the words go to stderr).
#include "common.h"
#include "native_common.h"

#include "y4m_host.cc"
#include "yuv_enc.hip"

static int run_encode(const char* in, const char* outp) {
  std::ifstream f(in, std::ios::binary);
  std::ofstream o(outp, std::ios::binary);
  int32_t count = 0;
  f.read((char*)&count, sizeof count);
  for (int c = 0; c < count; ++c) {
    int32_t hd[9];
    f.read((char*)hd, sizeof hd);
    if (!f) return 10;
    const int matrix = hd[0], full = hd[1], bgr = hd[2], chroma = hd[3], F = hd[4], H = hd[5], W = hd[6], oH = hd[7], oW = hd[8];
    const size_t src_bytes = (size_t)F * H * W * 3;
    std::vector<uint8_t> pixels(src_bytes);
    f.read((char*)pixels.data(), (std::streamsize)src_bytes);
    if (!f) return 11;
    pr_yuv_enc_args a;
    memset(&a, 0, sizeof a);
    if (pr_yuv_enc_plan(matrix, full, &a.plan) != PR_OK) return 12;
    a.F = F, a.H = H, a.W = W, a.out_H = oH, a.out_W = oW, a.chroma = chroma, a.bgr = bgr;
    pr_y4m_info info;
    memset(&info, 0, sizeof info);
    info.width = oW, info.height = oH, info.chroma = chroma, info.full_range = -1;
    const int cw = (chroma == PR_Y4M_C420JPEG || chroma == PR_Y4M_C420MPEG2 || chroma == PR_Y4M_C422) ? (oW + 1) / 2 : oW;
    const int ch = (chroma == PR_Y4M_C420JPEG || chroma == PR_Y4M_C420MPEG2) ? (oH + 1) / 2 : oH;
    info.frame_bytes = (int64_t)oW * oH + (chroma == PR_Y4M_CMONO ? 0 : 2 * (int64_t)cw * ch);
    const size_t total = (size_t)F * (6 + (size_t)info.frame_bytes);
    const int32_t total32 = (int32_t)total;
    o.write((const char*)&total32, sizeof total32);
    o.write((const char*)&a.plan, sizeof a.plan);
    std::vector<uint8_t> first;
    for (int dshift = 0; dshift < 4; ++dshift) {
      for (int sshift = 0; sshift < 4; ++sshift) {
        auto src = exact<uint8_t>(src_bytes + sshift);
        auto dst = exact<uint8_t>(total + dshift);
        if (((uintptr_t)src.get() | (uintptr_t)dst.get()) & 3) return 13;
        memset(src.get(), 0xCD, src_bytes + sshift);
        memcpy(src.get() + sshift, pixels.data(), src_bytes);
        memset(dst.get(), 0xAB, total + dshift);
        a.src = src.get() + sshift, a.dst = dst.get() + dshift;
        if (pr_yuv_encode(&a, nullptr) != PR_OK) return 14;
        for (int i = 0; i < dshift; ++i)
          if (dst[i] != 0xAB) {
            fprintf(stderr, "call %d, dst alignment %d: byte %d in front of the output was written\n", c, dshift, i);
            return 15;
          }
        if (memcmp(src.get() + sshift, pixels.data(), src_bytes)) return 16;      // reads only src
        if (first.empty()) first.assign(dst.get() + dshift, dst.get() + dshift + total);
        if (memcmp(first.data(), dst.get() + dshift, total)) {
          fprintf(stderr, "call %d: dst alignment %d, src alignment %d: other bytes than at alignments 0, 0\n", c, dshift, sshift);
          return 17;
        }
        if (sshift == ((dshift + 1) & 3)) o.write((const char*)dst.get() + dshift, (std::streamsize)total);
      }
    }
    // the output is a chunk of a valid stream
    auto offsets = exact<int64_t>((size_t)F + 1);
    int32_t n = -1;
    int64_t used = -1;
    if (pr_y4m_index(first.data(), (int64_t)total, &info, offsets.get(), F + 1, &n, &used) != PR_OK) return 18;
    if (n != F || used != (int64_t)total) return 19;
    for (int k = 0; k < F; ++k)
      if (offsets[k] != (int64_t)k * (6 + info.frame_bytes) + 6) return 20;
  }
  return 0;
}

static int run_refusals() {
  int bad = 0, count = 0;
  auto refused = [&](int rc) { ++count, bad += rc != PR_ERR_INVALID; };
  pr_yuv_enc_coeffs plan;
  memset(&plan, 0x5A, sizeof plan);
  const pr_yuv_enc_coeffs plan0 = plan;
  refused(pr_yuv_enc_plan(2, 0, &plan));
  refused(pr_yuv_enc_plan(-1, 0, &plan));
  refused(pr_yuv_enc_plan(0, 2, &plan));
  refused(pr_yuv_enc_plan(0, -1, &plan));
  refused(pr_yuv_enc_plan(0, 0, nullptr));
  if (memcmp(&plan, &plan0, sizeof plan)) return 30;            // a refused call writes nothing
  if (pr_yuv_enc_plan(PR_YUV_601, 0, &plan) != PR_OK || plan.kyr != 16829 || plan.kyg != 33039 || plan.kyb != 6416 || plan.kc != 28784 ||
      plan.kur != 9714 || plan.kug != 19070 || plan.kvb != 4681 || plan.kvg != 24103 || plan.yo != 16)
    return 31;

  const int H = 3, W = 5, F = 2;
  auto src = exact<uint8_t>((size_t)F * H * W * 3);
  const size_t total = (size_t)F * (6 + 4 * 6 + 2 * 3 * 2);           // padded to 6 x 4, 420
  auto dst = exact<uint8_t>(total);
  memset(dst.get(), 0xAB, total);
  pr_yuv_enc_args good;
  memset(&good, 0, sizeof good);
  good.src = src.get(), good.dst = dst.get(), good.plan = plan;
  good.F = F, good.H = H, good.W = W, good.out_H = H + 1, good.out_W = W + 1, good.chroma = PR_Y4M_C420MPEG2;
  pr_yuv_enc_args a;
  refused(pr_yuv_encode(nullptr, nullptr));
  a = good, a.F = -1;
  refused(pr_yuv_encode(&a, nullptr));
  a = good, a.H = 0, a.out_H = 0;
  refused(pr_yuv_encode(&a, nullptr));
  a = good, a.W = 4097, a.out_W = 4097;
  refused(pr_yuv_encode(&a, nullptr));
  a = good, a.H = 4096, a.out_H = 4097;                               // the padded side is a side too
  refused(pr_yuv_encode(&a, nullptr));
  a = good, a.out_H = H + 2;
  refused(pr_yuv_encode(&a, nullptr));
  a = good, a.out_H = H - 1;
  refused(pr_yuv_encode(&a, nullptr));
  a = good, a.out_W = W + 2;
  refused(pr_yuv_encode(&a, nullptr));
  a = good, a.out_W = W - 1;
  refused(pr_yuv_encode(&a, nullptr));
  a = good, a.chroma = 5;
  refused(pr_yuv_encode(&a, nullptr));
  a = good, a.chroma = -1;
  refused(pr_yuv_encode(&a, nullptr));
  a = good, a.src = nullptr;
  refused(pr_yuv_encode(&a, nullptr));
  a = good, a.dst = nullptr;
  refused(pr_yuv_encode(&a, nullptr));
  for (size_t i = 0; i < total; ++i)
    if (dst[i] != 0xAB) return 32;                                    // no refused call did device work
  a = good, a.F = 0, a.src = nullptr, a.dst = nullptr, a.H = -3;      // F = 0 is legal whatever else is given
  if (pr_yuv_encode(&a, nullptr) != PR_OK) return 33;
  if (pr_yuv_encode(&good, nullptr) != PR_OK) return 34;
  for (size_t i = 0; i < total; ++i)
    if (dst[i] == 0xAB) return 35;                                    // black frames hold 16 and 128 only: every byte written
  printf("yuv_enc_native: %d of %d bad calls refused\n", count - bad, count);
  return bad ? 40 : 0;
}

int main(int argc, char** argv) {
  if (argc >= 4 && !strcmp(argv[1], "encode")) return run_encode(argv[2], argv[3]);
  if (argc >= 2 && !strcmp(argv[1], "refusals")) return run_refusals();
  return 2;
}
