// csrc/jpeg_host.cc, csrc/jpeg.hip and csrc/jpeg_sync.hip on the host (see host_shim.h), built by
// tests/test_jpeg_sync_native.py with g++ under ASan + UBSan.
//   jpeg_sync_native each <pack> <out> <S> <R> [bgr]   every stream of the pack on its own: copied to an exact-size heap block,
//       parsed (F = 1), decoded by pr_jpeg_decode and by pr_jpeg_decode_sync (S, R: 0 = the default) into exact-size buffers.
//       pack: int64 F, int64 offsets[F+1], bytes.   out, per stream: int32 parse_status, counts[4], serial status, sync status
//       (-1 when not decoded), stats[4], then for an accepted stream the serial pixels and the sync pixels, u8[H,W,3] each.
//   jpeg_sync_native args <pack>   the first stream of the pack through every argument error of pr_jpeg_decode_sync: each
//       must return PR_ERR_INVALID and leave pixels, status, stats and workspace as they were.
#include "common.h"
#include "native_common.h"

#include "jpeg_host.cc"
#include "jpeg.hip"
#include "jpeg_sync.hip"

struct Parsed {
  std::unique_ptr<uint8_t[]> data;
  int64_t n = 0;
  pr_jpeg_frame fr;
  int32_t st = -1, counts[4] = {0, 0, 0, 0};
  std::unique_ptr<pr_jpeg_segment[]> segs;
  std::unique_ptr<pr_jpeg_huff[]> huff;
  int rc = 0;
};

static void parse_one(const Pack& k, int64_t i, Parsed& q) {
  q.n = k.size(i);
  q.data = k.copy(i);
  const int64_t offsets[2] = {0, q.n};
  int rc = pr_jpeg_parse(q.data.get(), offsets, 1, 0, 0, &q.fr, nullptr, 0, nullptr, 0, &q.st, q.counts);
  if (rc != PR_OK && rc != PR_ERR_CAPACITY) {
    q.rc = 10;
    return;
  }
  const int nseg = q.counts[0], nhuff = q.counts[1];
  q.segs = exact<pr_jpeg_segment>((size_t)nseg);
  q.huff = exact<pr_jpeg_huff>((size_t)nhuff);
  if (q.st == PR_JPEG_OK) {
    rc = pr_jpeg_parse(q.data.get(), offsets, 1, 0, 0, &q.fr, q.segs.get(), nseg, q.huff.get(), nhuff, &q.st, q.counts);
    if (rc != PR_OK || q.st != PR_JPEG_OK || q.counts[0] != nseg || nhuff != 1) q.rc = 11;
  }
}

static pr_jpeg_args args_of(const Parsed& q, uint8_t* px, int32_t* status, int bgr) {
  pr_jpeg_args a{};
  a.data = q.data.get();
  a.frames = &q.fr;
  a.segments = q.segs.get();
  a.huff = q.huff.get();
  a.out = px;
  a.status = status;
  a.data_bytes = q.n;
  a.F = 1;
  a.H = q.counts[2];
  a.W = q.counts[3];
  a.n_segments = q.counts[0];
  a.n_huff = q.counts[1];
  a.bgr = bgr;
  return a;
}

static int run_each(const char* in, const char* outp, int S, int R, int bgr) {
  const Pack k = read_pack(in);
  std::ofstream o(outp, std::ios::binary);
  const pr_jpeg_sync_opts given = {S, R};
  const pr_jpeg_sync_opts* opts = S || R ? &given : nullptr;   // 0 0 = the build's defaults
  for (int64_t i = 0; i < k.F; ++i) {
    Parsed q;
    parse_one(k, i, q);
    if (q.rc) return q.rc;
    int32_t serial_st = -1, sync_st = -1;
    pr_jpeg_sync_stats stats = {-1, -1, -1, -1};
    std::unique_ptr<uint8_t[]> px, px2;
    size_t px_bytes = 0;
    if (q.st == PR_JPEG_OK) {
      const int H = q.counts[2], W = q.counts[3];
      px_bytes = (size_t)H * W * 3;
      px = exact<uint8_t>(px_bytes);
      px2 = exact<uint8_t>(px_bytes);
      memset(px.get(), 0xAB, px_bytes);
      memset(px2.get(), 0xAB, px_bytes);
      {
        const size_t ws_bytes = pr_jpeg_workspace_bytes(1, H, W);
        auto ws = exact<uint8_t>(ws_bytes);
        memset(ws.get(), 0xCD, ws_bytes);
        const pr_jpeg_args a = args_of(q, px.get(), &serial_st, bgr);
        if (pr_jpeg_decode(&a, ws.get(), ws_bytes, nullptr) != PR_OK) return 13;
      }
      const size_t ws_bytes = pr_jpeg_sync_workspace_bytes(1, H, W, q.n, q.counts[0], opts);
      if (!ws_bytes) return 14;
      auto ws = exact<uint8_t>(ws_bytes);   // 16-byte aligned: operator new[] gives that
      memset(ws.get(), 0xCD, ws_bytes);
      const pr_jpeg_args a = args_of(q, px2.get(), &sync_st, bgr);
      if (pr_jpeg_decode_sync(&a, opts, &stats, ws.get(), ws_bytes, nullptr) != PR_OK) return 15;
    }
    o.write((char*)&q.st, 4);
    o.write((char*)q.counts, 16);
    o.write((char*)&serial_st, 4);
    o.write((char*)&sync_st, 4);
    o.write((char*)&stats, 16);
    if (q.st == PR_JPEG_OK) {
      o.write((char*)px.get(), (std::streamsize)px_bytes);
      o.write((char*)px2.get(), (std::streamsize)px_bytes);
    }
  }
  printf("jpeg_sync_native: %lld streams\n", (long long)k.F);
  return 0;
}

static int run_args(const char* in) {
  const Pack k = read_pack(in);
  Parsed q;
  parse_one(k, 0, q);
  if (q.rc || q.st != PR_JPEG_OK) return 20;
  const int H = q.counts[2], W = q.counts[3];
  const size_t px_bytes = (size_t)H * W * 3;
  const pr_jpeg_sync_opts good = {0, 8};
  const size_t ws_bytes = pr_jpeg_sync_workspace_bytes(1, H, W, q.n, q.counts[0], &good);
  if (!ws_bytes) return 21;
  auto px = exact<uint8_t>(px_bytes);
  auto ws = exact<uint8_t>(ws_bytes + 16);
  int32_t status = 0x5A5A5A5A;
  pr_jpeg_sync_stats stats = {0x5A, 0x5A, 0x5A, 0x5A};
  memset(px.get(), 0xAB, px_bytes);
  memset(ws.get(), 0xCD, ws_bytes + 16);
  int failures = 0, tried = 0;
  auto untouched = [&]() {
    for (size_t i = 0; i < px_bytes; ++i)
      if (px[i] != 0xAB) return false;
    for (size_t i = 0; i < ws_bytes + 16; ++i)
      if (ws[i] != 0xCD) return false;
    return status == 0x5A5A5A5A && stats.n_subseq == 0x5A && stats.rounds == 0x5A && stats.fell_back == 0x5A && stats.reserved == 0x5A;
  };
  auto expect_invalid = [&](const char* what, const pr_jpeg_args* a, const pr_jpeg_sync_opts* o, void* w, size_t wb) {
    ++tried;
    const int rc = pr_jpeg_decode_sync(a, o, &stats, w, wb, nullptr);
    if (rc != PR_ERR_INVALID || !untouched()) {
      fprintf(stderr, "argument error '%s': returned %d, buffers %s\n", what, rc, untouched() ? "untouched" : "WRITTEN");
      ++failures;
    }
  };
  const pr_jpeg_args a = args_of(q, px.get(), &status, 0);
  expect_invalid("null args", nullptr, &good, ws.get(), ws_bytes);
  expect_invalid("null workspace", &a, &good, nullptr, ws_bytes);
  pr_jpeg_args b = a;
  b.frames = nullptr;
  expect_invalid("null frames", &b, &good, ws.get(), ws_bytes);
  b = a;
  b.out = nullptr;
  expect_invalid("null out", &b, &good, ws.get(), ws_bytes);
  b = a;
  b.status = nullptr;
  expect_invalid("null status", &b, &good, ws.get(), ws_bytes);
  b = a;
  b.data = nullptr;
  expect_invalid("null data", &b, &good, ws.get(), ws_bytes);
  b = a;
  b.segments = nullptr;
  expect_invalid("null segments", &b, &good, ws.get(), ws_bytes);
  b = a;
  b.huff = nullptr;
  expect_invalid("null huff", &b, &good, ws.get(), ws_bytes);
  const int bad_s[3] = {12, 18, 8192}, bad_r[2] = {0, 65};
  for (int s : bad_s) {
    const pr_jpeg_sync_opts o = {s, 8};
    expect_invalid("subseq_bytes", &a, &o, ws.get(), ws_bytes);
    ++tried;
    if (pr_jpeg_sync_workspace_bytes(1, H, W, q.n, q.counts[0], &o) != 0) ++failures;
  }
  for (int r : bad_r) {
    const pr_jpeg_sync_opts o = {0, r};
    expect_invalid("max_rounds", &a, &o, ws.get(), ws_bytes);
    ++tried;
    if (pr_jpeg_sync_workspace_bytes(1, H, W, q.n, q.counts[0], &o) != 0) ++failures;
  }
  expect_invalid("workspace one byte short", &a, &good, ws.get(), ws_bytes - 1);
  expect_invalid("workspace misaligned", &a, &good, ws.get() + 8, ws_bytes);
  printf("jpeg_sync_native: %d argument errors tried, %d wrong\n", tried, failures);
  return failures ? 22 : 0;
}

int main(int argc, char** argv) {
  if (argc >= 6 && !strcmp(argv[1], "each")) return run_each(argv[2], argv[3], atoi(argv[4]), atoi(argv[5]), argc > 6 ? atoi(argv[6]) : 0);
  if (argc >= 3 && !strcmp(argv[1], "args")) return run_args(argv[2]);
  return 2;
}
