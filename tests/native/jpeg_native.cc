// csrc/jpeg_host.cc and csrc/jpeg.hip on the host (see host_shim.h), built by tests/test_jpeg_native.py with
// g++ under ASan + UBSan.
//   jpeg_native each <pack> <out> [bgr]   every stream of the pack on its own: copied to an exact-size heap block, parsed
//       (F = 1), its segment ranges checked against the block, decoded into exact-size buffers.
//       pack: int64 F, int64 offsets[F+1], bytes.   out, per stream: int32 parse_status, counts[4], decode_status (-1 when not
//       decoded), then for an accepted stream pr_jpeg_frame, its segments, its pr_jpeg_huff, the pixels u8[H,W,3].
//   jpeg_native idct <in> <out>   the IDCT kernel alone on four hand-made blocks of a 16x16 one-component frame.
//       in: int16 coef[4][64] (natural order), uint16 quant[64].   out: u8 plane[16][16], int32 status.
#include "common.h"
#include "native_common.h"

#include "jpeg_host.cc"
#include "jpeg.hip"

static int run_each(const char* in, const char* outp, int bgr) {
  const Pack k = read_pack(in);
  const int64_t F = k.F;
  std::ofstream o(outp, std::ios::binary);
  for (int64_t i = 0; i < F; ++i) {
    const int64_t n = k.size(i);
    auto data = k.copy(i);
    const int64_t offsets[2] = {0, n};
    pr_jpeg_frame fr;
    int32_t st = -1, counts[4] = {0, 0, 0, 0}, dst = -1;
    // first call: how many segments; second call: exactly that many
    int rc = pr_jpeg_parse(data.get(), offsets, 1, 0, 0, &fr, nullptr, 0, nullptr, 0, &st, counts);
    if (rc != PR_OK && rc != PR_ERR_CAPACITY) return 10;
    const int nseg = counts[0], nhuff = counts[1];
    auto segs = exact<pr_jpeg_segment>((size_t)nseg);
    auto huff = exact<pr_jpeg_huff>((size_t)nhuff);
    if (st == PR_JPEG_OK) {
      rc = pr_jpeg_parse(data.get(), offsets, 1, 0, 0, &fr, segs.get(), nseg, huff.get(), nhuff, &st, counts);
      if (rc != PR_OK || st != PR_JPEG_OK || counts[0] != nseg || nhuff != 1) return 11;
      for (int s = 0; s < nseg; ++s)
        if (segs[s].begin < 0 || segs[s].begin > segs[s].end || segs[s].end > n || segs[s].frame != 0) {
          fprintf(stderr, "stream %lld: segment %d = [%lld, %lld) leaves the %lld bytes\n", (long long)i, s,
                  (long long)segs[s].begin, (long long)segs[s].end, (long long)n);
          return 12;
        }
    }
    std::unique_ptr<uint8_t[]> px;
    size_t px_bytes = 0;
    if (st == PR_JPEG_OK) {
      const int H = counts[2], W = counts[3];
      px_bytes = (size_t)H * W * 3;
      // the workspace must be 16-byte aligned: operator new[] gives that
      px = exact<uint8_t>(px_bytes);
      const size_t ws_bytes = pr_jpeg_workspace_bytes(1, H, W);
      auto ws = exact<uint8_t>(ws_bytes);
      memset(ws.get(), 0xCD, ws_bytes);
      memset(px.get(), 0xAB, px_bytes);
      pr_jpeg_args a{};
      a.data = data.get();
      a.frames = &fr;
      a.segments = segs.get();
      a.huff = huff.get();
      a.out = px.get();
      a.status = &dst;
      a.data_bytes = n;
      a.F = 1;
      a.H = H;
      a.W = W;
      a.n_segments = nseg;
      a.n_huff = nhuff;
      a.bgr = bgr;
      if (pr_jpeg_decode(&a, ws.get(), ws_bytes, nullptr) != PR_OK) return 13;
    }
    o.write((char*)&st, 4);
    o.write((char*)counts, 16);
    o.write((char*)&dst, 4);
    if (st == PR_JPEG_OK) {
      o.write((char*)&fr, sizeof fr);
      o.write((char*)segs.get(), (std::streamsize)(sizeof(pr_jpeg_segment) * nseg));
      o.write((char*)huff.get(), sizeof(pr_jpeg_huff));
      o.write((char*)px.get(), (std::streamsize)px_bytes);
    }
  }
  printf("jpeg_native: %lld streams\n", (long long)F);
  return 0;
}

static int run_idct(const char* in, const char* outp) {
  using namespace pr;
  std::ifstream f(in, std::ios::binary);
  const long cs = padded_samples(16, 16);
  auto coef = exact<short>((size_t)cs);
  auto planes = exact<unsigned char>((size_t)cs);
  pr_jpeg_frame fr;
  memset(&fr, 0, sizeof fr);
  f.read((char*)coef.get(), 4 * 64 * 2);
  f.read((char*)fr.quant[0], 128);
  fr.width = fr.height = 16;
  fr.ncomp = fr.hs = fr.vs = 1;
  pr_jpeg_huff huff;
  memset(&huff, 0, sizeof huff);
  int32_t status = 0;
  JpegParams p;
  memset(&p, 0, sizeof p);
  p.a.frames = &fr;
  p.a.huff = &huff;
  p.a.status = &status;
  p.a.F = 1;
  p.a.H = p.a.W = 16;
  p.a.n_huff = 1;
  p.coef = coef.get();
  p.planes = planes.get();
  p.cs = cs;
  hipLaunchKernelGGL(jpeg_idct_kernel, dim3((unsigned)ceil_div(cs / 64, (long)kThreads), 1u), dim3(kThreads), 0, nullptr, p);
  std::ofstream o(outp, std::ios::binary);
  o.write((char*)planes.get(), 256);
  o.write((char*)&status, 4);
  return 0;
}

int main(int argc, char** argv) {
  if (argc >= 4 && !strcmp(argv[1], "each")) return run_each(argv[2], argv[3], argc > 4 ? atoi(argv[4]) : 0);
  if (argc >= 4 && !strcmp(argv[1], "idct")) return run_idct(argv[2], argv[3]);
  return 2;
}
