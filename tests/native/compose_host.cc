// csrc/compose.hip on the host (see host_shim.h): reads a case file, runs pr_compose_video, writes the canvases.
//   case file: int32 header[24] = N n_frames H W dst_h dst_w panel_w L C S CH CW adv[4] ascent[4] box_rgb[3] has_src_idx,
//   then frames, src_idx, box, lines, text, atlas as raw bytes.   usage: compose_host <case> <out> [output misalignment]
#define HOST_SHIM_THREADS      // compose.hip meets at barriers ...
#define HOST_SHIM_SHARED       // ... and declares its LDS block extern: it is the array below
#include "common.h"
#include "native_common.h"

unsigned pr_compose_lds[kLdsBytes / 4] __attribute__((aligned(16)));
#include "compose.hip"

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  std::ifstream f(argv[1], std::ios::binary);
  int h[24];
  f.read((char*)h, sizeof h);
  pr_compose_args a{};
  a.N = h[0]; a.n_frames = h[1]; a.H = h[2]; a.W = h[3]; a.dst_h = h[4]; a.dst_w = h[5]; a.panel_w = h[6];
  a.L = h[7]; a.C = h[8]; a.S = h[9]; a.CH = h[10]; a.CW = h[11];
  for (int i = 0; i < 4; ++i) { a.adv[i] = h[12 + i]; a.ascent[i] = h[16 + i]; }
  for (int i = 0; i < 3; ++i) a.box_rgb[i] = (uint8_t)h[20 + i];
  // exact-size heap blocks: the sanitizer sees any byte read or written outside them
  std::vector<std::unique_ptr<uint8_t[]>> blocks;
  auto rd = [&](size_t n) {
    blocks.emplace_back(new uint8_t[n ? n : 1]);
    f.read((char*)blocks.back().get(), (std::streamsize)n);
    return blocks.back().get();
  };
  a.frames = rd((size_t)a.n_frames * a.H * a.W * 3);
  a.src_idx = (const int32_t*)rd((size_t)a.N * 4);
  if (!h[23]) a.src_idx = nullptr;
  a.box = (const int32_t*)rd((size_t)a.N * 16);
  a.lines = (const int32_t*)rd((size_t)a.N * a.L * PR_VIDEO_LINE_INTS * 4);
  a.text = rd((size_t)a.N * a.L * a.C);
  a.atlas = rd((size_t)a.S * 96 * a.CH * a.CW);
  const size_t out_bytes = (size_t)a.N * a.dst_h * (a.dst_w + a.panel_w) * 3;
  const int shift = argc > 3 ? atoi(argv[3]) : 0;
  std::unique_ptr<uint8_t[]> out(new uint8_t[out_bytes + shift]);
  memset(out.get(), 0xAB, out_bytes + shift);
  std::vector<int32_t> status(a.N, -7);
  a.out = out.get() + shift;
  a.status = status.data();
  const int rc = pr_compose_video(&a, nullptr);
  if (g_lds_asked > kLdsBytes) {
    fprintf(stderr, "the launch asked for %zu bytes of LDS\n", g_lds_asked);
    return 3;
  }
  for (int i = 0; i < shift; ++i)
    if (out[i] != 0xAB) { fprintf(stderr, "byte %d in front of out was written\n", i); return 4; }
  std::ofstream o(argv[2], std::ios::binary);
  o.write((char*)a.out, (std::streamsize)out_bytes);
  o.write((char*)status.data(), (std::streamsize)a.N * 4);
  printf("compose_host: status %d, %zu bytes of LDS\n", rc, g_lds_asked);
  return rc == 0 ? 0 : 1;
}
