// csrc/jpeg_host.cc and csrc/jpeg_enc.hip on the host (see host_shim.h), built by tests/test_jpeg_encode_native.py with
// g++ under ASan + UBSan.
//   jpeg_enc_native encode <in> <out>   F frames through pr_jpeg_encode_plan and pr_jpeg_encode, once per capacity, every buffer
//       an exact-size heap block.  in: int32 F, H, W, hs, vs, restart_interval, quality, bgr, ncap; int64 capacity[ncap] (-1 = the
//       bound); u8 frames[F,H,W,3].   out, per capacity: int64 capacity used, int32 nbytes[F], int32 status[F], u8 out[F,capacity]
//       (0xAB where nothing was written); then once the plan (pr_jpeg_enc_plan) and int64 bound.
//   jpeg_enc_native quant   the reciprocal quantiser against the division for every magnitude 0..16384, both signs, and every
//       divisor 8..2040.
//   jpeg_enc_native fdct <in> <out>   in: int32 n, int32 samples[n][64] (0..255).  out: int32 coefficients[n][64] of the 32-bit FDCT.
#include "common.h"
#include "native_common.h"

#include "jpeg_host.cc"
#include "jpeg_enc.hip"

static int run_encode(const char* in, const char* outp) {
  std::ifstream f(in, std::ios::binary);
  int32_t h[9];
  f.read((char*)h, sizeof h);
  const int F = h[0], H = h[1], W = h[2], hs = h[3], vs = h[4], ri = h[5], quality = h[6], bgr = h[7], ncap = h[8];
  std::vector<int64_t> caps((size_t)ncap);
  f.read((char*)caps.data(), (std::streamsize)(8 * ncap));
  const size_t px_bytes = (size_t)F * H * W * 3;
  auto frames = exact<uint8_t>(px_bytes);
  f.read((char*)frames.get(), (std::streamsize)px_bytes);
  if (!f) return 10;
  auto plan = exact<pr_jpeg_enc_plan>(1);
  if (pr_jpeg_encode_plan(quality, hs, vs, ri, H, W, plan.get()) != PR_OK) return 11;
  const int64_t bound = (int64_t)pr_jpeg_encode_bound(H, W, hs, vs, ri);
  std::ofstream o(outp, std::ios::binary);
  for (int64_t cap : caps) {
    if (cap < 0) cap = bound;
    const size_t ws_bytes = pr_jpeg_encode_workspace_bytes(F, H, W, hs, vs, ri, cap);
    if (!ws_bytes) return 12;
    auto ws = exact<uint8_t>(ws_bytes);   // operator new[] gives the 16-byte alignment the entry asks for
    memset(ws.get(), 0xCD, ws_bytes);
    auto out = exact<uint8_t>((size_t)F * cap);
    memset(out.get(), 0xAB, (size_t)F * cap);
    auto nbytes = exact<int32_t>((size_t)F), status = exact<int32_t>((size_t)F);
    for (int i = 0; i < F; ++i) nbytes[i] = status[i] = -7;
    pr_jpeg_enc_args a{};
    a.frames = frames.get();
    a.plan = plan.get();
    a.out = out.get();
    a.nbytes = nbytes.get();
    a.status = status.get();
    a.capacity = cap;
    a.F = F;
    a.H = H;
    a.W = W;
    a.hs = hs;
    a.vs = vs;
    a.restart_interval = ri;
    a.bgr = bgr;
    if (pr_jpeg_encode(&a, ws.get(), ws_bytes, nullptr) != PR_OK) return 13;
    o.write((char*)&cap, 8);
    o.write((char*)nbytes.get(), 4 * F);
    o.write((char*)status.get(), 4 * F);
    o.write((char*)out.get(), (std::streamsize)((size_t)F * cap));
  }
  o.write((char*)plan.get(), sizeof(pr_jpeg_enc_plan));
  o.write((char*)&bound, 8);
  return 0;
}

static int run_quant() {
  long checked = 0;
  for (unsigned q8 = 8; q8 <= 2040; ++q8) {
    const unsigned recip = pr::enc_recip(q8);
    for (int m = 0; m <= 16384; ++m) {
      const int want = (int)((m + (q8 >> 1)) / q8);
      if (pr::enc_quantise(m, q8, recip) != want || pr::enc_quantise(-m, q8, recip) != -want) {
        fprintf(stderr, "quantiser: %d / %u gives %d and %d, the division %d\n", m, q8, pr::enc_quantise(m, q8, recip),
                pr::enc_quantise(-m, q8, recip), want);
        return 20;
      }
      checked += 2;
    }
  }
  printf("jpeg_enc_native: %ld quotients equal the division\n", checked);
  return 0;
}

static int run_fdct(const char* in, const char* outp) {
  std::ifstream f(in, std::ios::binary);
  int32_t n = 0;
  f.read((char*)&n, 4);
  auto blocks = exact<int32_t>((size_t)n * 64);
  f.read((char*)blocks.get(), (std::streamsize)((size_t)n * 256));
  if (!f) return 30;
  for (int i = 0; i < n; ++i) {
    int d[64];
    for (int j = 0; j < 64; ++j) d[j] = blocks[(size_t)i * 64 + j] - 128;
    pr::fdct8x8(d);
    for (int j = 0; j < 64; ++j) blocks[(size_t)i * 64 + j] = d[j];
  }
  std::ofstream o(outp, std::ios::binary);
  o.write((char*)blocks.get(), (std::streamsize)((size_t)n * 256));
  return 0;
}

int main(int argc, char** argv) {
  if (argc >= 4 && !strcmp(argv[1], "encode")) return run_encode(argv[2], argv[3]);
  if (argc >= 2 && !strcmp(argv[1], "quant")) return run_quant();
  if (argc >= 4 && !strcmp(argv[1], "fdct")) return run_fdct(argv[2], argv[3]);
  return 2;
}
