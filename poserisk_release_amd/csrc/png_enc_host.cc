// Host half of the PNG encoder (include/poserisk_hip.h, section j5): the plan -- the fixed bytes of a file and the CRC power
// table -- the capacity bound and the workspace size.  Device-free, like png_host.cc: it is compiled without the offload pass,
// and by g++ under sanitizers for tests/test_png_encode_native.py.
#include "host_common.h"
#define PR_PNG_ENC_HOST_ONLY
#include "png_enc_device.h"

namespace pr {
namespace {

uint32_t crc_of(const uint8_t* p, size_t n, uint32_t c) {   // the register, not inverted
  for (size_t i = 0; i < n; ++i) c = pngenc::crc_byte(c, p[i]);
  return c;
}

void put_be32(uint8_t* p, uint32_t v) {
  p[0] = (uint8_t)(v >> 24), p[1] = (uint8_t)(v >> 16), p[2] = (uint8_t)(v >> 8), p[3] = (uint8_t)v;
}

}  // namespace
}  // namespace pr

extern "C" size_t pr_png_encode_bound(int H, int W) {
  if (H < 1 || W < 1 || H > PR_PNG_MAX_SIDE || W > PR_PNG_MAX_SIDE) return 0;
  const size_t raw = (size_t)H * (1 + 3 * (size_t)W);
  return PR_PNG_ENC_HEAD_BYTES + 4 + 4 + PR_PNG_ENC_TAIL_BYTES + raw + 5 * ((raw + PR_PNG_ENC_SEGMENT - 1) / PR_PNG_ENC_SEGMENT);
}

extern "C" size_t pr_png_encode_workspace_bytes(int F, int H, int W) {
  pr::pngenc::EncLayout l;
  return pr::pngenc::enc_layout(F, H, W, &l) ? l.total : 0;
}

extern "C" int pr_png_encode_plan(int filter, int mode, int H, int W, pr_png_enc_plan* plan) {
  using namespace pr;
  PR_REQUIRE(plan, "pr_png_encode_plan: null plan");
  PR_REQUIRE(filter >= 0 && filter <= PR_PNG_ENC_FILTER_ADAPTIVE, "pr_png_encode_plan: filter %d is not 0..4 or 5 (adaptive)", filter);
  PR_REQUIRE(mode == PR_PNG_ENC_STORED || mode == PR_PNG_ENC_RLE, "pr_png_encode_plan: mode %d is neither PR_PNG_ENC_STORED nor PR_PNG_ENC_RLE", mode);
  PR_REQUIRE(H >= 1 && W >= 1 && H <= PR_PNG_MAX_SIDE && W <= PR_PNG_MAX_SIDE, "pr_png_encode_plan: size %d x %d is outside 1..%d", W, H,
             PR_PNG_MAX_SIDE);
  memset(plan, 0, sizeof *plan);
  plan->width = W, plan->height = H, plan->filter = filter, plan->mode = mode;
  plan->raw_bytes = (int64_t)H * (1 + 3 * (int64_t)W);
  plan->n_segments = (int32_t)((plan->raw_bytes + PR_PNG_ENC_SEGMENT - 1) / PR_PNG_ENC_SEGMENT);
  uint32_t p = 1u << 30;   // x^1
  plan->crc_pow[0] = p;
  for (int k = 1; k < 32; ++k) plan->crc_pow[k] = p = pngenc::multmodp(p, p);
  static const uint8_t sig[8] = {0x89, 'P', 'N', 'G', '\r', '\n', 0x1a, '\n'};
  uint8_t* h = plan->head;
  memcpy(h, sig, 8);
  put_be32(h + 8, 13);
  memcpy(h + 12, "IHDR", 4);
  put_be32(h + 16, (uint32_t)W);
  put_be32(h + 20, (uint32_t)H);
  h[24] = 8, h[25] = 2, h[26] = 0, h[27] = 0, h[28] = 0;   // depth 8, colour type 2, deflate, filter method 0, no interlace
  put_be32(h + 29, ~crc_of(h + 12, 17, 0xFFFFFFFFu));
  memcpy(h + 37, "IDAT", 4);                                // h[33..36]: IDAT's length, written on the device
  h[41] = 0x78, h[42] = 0x01;
  plan->idat_crc_head = crc_of(h + 37, 6, 0xFFFFFFFFu);
  uint8_t* t = plan->tail;
  put_be32(t, 0);
  memcpy(t + 4, "IEND", 4);
  put_be32(t + 8, ~crc_of(t + 4, 4, 0xFFFFFFFFu));
  return PR_OK;
}
