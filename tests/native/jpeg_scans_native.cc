// csrc/jpeg_scans_host.cc and csrc/jpeg_scans.hip (with csrc/jpeg_host.cc and csrc/jpeg.hip behind them) on the host, built by
// tests/test_jpeg_scans_native.py with g++ under ASan + UBSan, each source its own translation unit.
//   jpeg_scans_native each <pack> <out> [bgr]   every stream of the pack on its own: copied to an exact-size heap block, parsed
//       by pr_jpeg_parse_scans (F = 1; once for the counts, once into arrays of exactly that size), its segment ranges checked
//       against the block, decoded by pr_jpeg_decode_scans into exact-size buffers.
//       pack: int64 F, int64 offsets[F+1], bytes.   out, per stream: int32 parse_status, counts[8], decode_status (-1 when not
//       decoded), then for an accepted stream pr_jpeg_frame, its segments, their scan indices, its scans, its table sets, the
//       pixels u8[H,W,3].
#include "common.h"
#include "native_common.h"

int main(int argc, char** argv) {
  if (argc < 4 || strcmp(argv[1], "each")) return 2;
  const int bgr = argc > 4 ? atoi(argv[4]) : 0;
  const Pack k = read_pack(argv[2]);
  const int64_t F = k.F;
  std::ofstream o(argv[3], std::ios::binary);
  for (int64_t i = 0; i < F; ++i) {
    const int64_t n = k.size(i);
    auto data = k.copy(i);
    const int64_t offsets[2] = {0, n};
    pr_jpeg_frame fr;
    int32_t st = -1, counts[8] = {0, 0, 0, 0, 0, 0, 0, 0}, dst = -1;
    int rc = pr_jpeg_parse_scans(data.get(), offsets, 1, 0, 0, &fr, nullptr, nullptr, 0, nullptr, 0, nullptr, 0, &st, counts);
    if (rc != PR_OK && rc != PR_ERR_CAPACITY) return 10;
    const int nseg = counts[0], nhuff = counts[1], nscan = counts[4];
    auto segs = exact<pr_jpeg_segment>((size_t)nseg);
    auto seg_scan = exact<int32_t>((size_t)nseg);
    auto huff = exact<pr_jpeg_huff>((size_t)nhuff);
    auto scans = exact<pr_jpeg_scan>((size_t)nscan);
    std::unique_ptr<uint8_t[]> px;
    size_t px_bytes = 0;
    if (st == PR_JPEG_OK) {
      rc = pr_jpeg_parse_scans(data.get(), offsets, 1, 0, 0, &fr, segs.get(), seg_scan.get(), nseg, huff.get(), nhuff, scans.get(),
                               nscan, &st, counts);
      if (rc != PR_OK || st != PR_JPEG_OK || counts[0] != nseg || counts[1] != nhuff || counts[4] != nscan) return 11;
      for (int s = 0; s < nseg; ++s)
        if (segs[s].begin < 0 || segs[s].begin > segs[s].end || segs[s].end > n || segs[s].frame != 0 || seg_scan[s] < 0 ||
            seg_scan[s] >= nscan) {
          fprintf(stderr, "stream %lld: segment %d = [%lld, %lld) of scan %d leaves the %lld bytes or the %d scans\n", (long long)i,
                  s, (long long)segs[s].begin, (long long)segs[s].end, seg_scan[s], (long long)n, nscan);
          return 12;
        }
      const int H = counts[2], W = counts[3];
      px_bytes = (size_t)H * W * 3;
      px = exact<uint8_t>(px_bytes);
      const size_t ws_bytes = pr_jpeg_scans_workspace_bytes(1, H, W);
      auto ws = exact<uint8_t>(ws_bytes);   // operator new[] gives the 16-byte alignment the workspace needs
      memset(ws.get(), 0xCD, ws_bytes);
      memset(px.get(), 0xAB, px_bytes);
      pr_jpeg_scans_args a{};
      a.base.data = data.get();
      a.base.frames = &fr;
      a.base.segments = segs.get();
      a.base.huff = huff.get();
      a.base.out = px.get();
      a.base.status = &dst;
      a.base.data_bytes = n;
      a.base.F = 1;
      a.base.H = H;
      a.base.W = W;
      a.base.n_segments = nseg;
      a.base.n_huff = nhuff;
      a.base.bgr = bgr;
      a.scans = scans.get();
      a.segment_scan = seg_scan.get();
      a.n_scans = nscan;
      a.n_levels = counts[5];
      if (pr_jpeg_decode_scans(&a, ws.get(), ws_bytes, nullptr) != PR_OK) return 13;
    }
    o.write((char*)&st, 4);
    o.write((char*)counts, 32);
    o.write((char*)&dst, 4);
    if (st == PR_JPEG_OK) {
      o.write((char*)&fr, sizeof fr);
      o.write((char*)segs.get(), (std::streamsize)(sizeof(pr_jpeg_segment) * nseg));
      o.write((char*)seg_scan.get(), (std::streamsize)(4 * nseg));
      o.write((char*)scans.get(), (std::streamsize)(sizeof(pr_jpeg_scan) * nscan));
      o.write((char*)huff.get(), (std::streamsize)(sizeof(pr_jpeg_huff) * nhuff));
      o.write((char*)px.get(), (std::streamsize)px_bytes);
    }
  }
  printf("jpeg_scans_native: %lld streams\n", (long long)F);
  return 0;
}
