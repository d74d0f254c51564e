// csrc/compose.hip on the host (see host_shim.h): reads a case file, runs pr_compose_people, writes the canvases.
//   case file: int32 header[24] = N n_frames H W dst_h dst_w panel_w K L L_img C S CH CW adv[4] ascent[4] has_src_idx has_box,
//   then frames, src_idx, box, box_rgb, lines, text, atlas as raw bytes.
//   usage: compose_people_host <case> <out> [output misalignment]
//          compose_people_host --validate      every argument error: PR_ERR_INVALID, `out` untouched, no launch
#define HOST_SHIM_THREADS      // compose.hip meets at barriers ...
#define HOST_SHIM_SHARED       // ... and declares its LDS block extern: it is the array below
#define NATIVE_QUIET_ERRORS    // --validate provokes every refusal and reads its message
#include "common.h"
#include "native_common.h"

unsigned pr_compose_lds[kLdsBytes / 4] __attribute__((aligned(16)));
using pr::g_error;
#include "compose.hip"

static int validate() {
  // a valid 1-canvas call on exact-size buffers, then one field wrong at a time
  const int H = 5, W = 7, dst_h = 4, dst_w = 6, panel_w = 3, K = 2, L = 3, C = 2, S = 1, CH = 3, CW = 2;
  std::vector<uint8_t> frames(H * W * 3, 9), rgb(K * 4, 200), text(L * C, 65), atlas(S * 96 * CH * CW, 128);
  std::vector<int32_t> box = {1, 1, 4, 3, 0, 0, -1, -1}, lines(L * PR_VIDEO_LINE_INTS, 0);
  const size_t out_bytes = (size_t)dst_h * (dst_w + panel_w) * 3;
  std::vector<uint8_t> out(out_bytes, 0xAB);
  pr_compose_people_args ok{};
  ok.frames = frames.data(); ok.box = box.data(); ok.box_rgb = rgb.data(); ok.lines = lines.data(); ok.text = text.data();
  ok.atlas = atlas.data(); ok.out = out.data();
  ok.N = 1; ok.n_frames = 1; ok.H = H; ok.W = W; ok.dst_h = dst_h; ok.dst_w = dst_w; ok.panel_w = panel_w;
  ok.K = K; ok.L = L; ok.L_img = 1; ok.C = C; ok.S = S; ok.CH = CH; ok.CW = CW; ok.adv[0] = 2; ok.ascent[0] = 2;
  struct Bad {
    const char* what;
    void (*set)(pr_compose_people_args&);
  };
  const Bad bad[] = {
      {"N < 0", [](pr_compose_people_args& a) { a.N = -1; }},
      {"null out", [](pr_compose_people_args& a) { a.out = nullptr; }},
      {"null frames", [](pr_compose_people_args& a) { a.frames = nullptr; }},
      {"n_frames 0", [](pr_compose_people_args& a) { a.n_frames = 0; }},
      {"H 0", [](pr_compose_people_args& a) { a.H = 0; }},
      {"W 4097", [](pr_compose_people_args& a) { a.W = 4097; }},
      {"dst_w 0", [](pr_compose_people_args& a) { a.dst_w = 0; }},
      {"dst_h 4097", [](pr_compose_people_args& a) { a.dst_h = 4097; }},
      {"panel_w -1", [](pr_compose_people_args& a) { a.panel_w = -1; }},
      {"K 0", [](pr_compose_people_args& a) { a.K = 0; }},
      {"K 17", [](pr_compose_people_args& a) { a.K = PR_PEOPLE_MAX_BOXES + 1; }},
      {"box without box_rgb", [](pr_compose_people_args& a) { a.box_rgb = nullptr; }},
      {"L 33", [](pr_compose_people_args& a) { a.L = PR_PEOPLE_MAX_LINES + 1; }},
      {"L -1", [](pr_compose_people_args& a) { a.L = -1; a.L_img = 0; }},
      {"L_img -1", [](pr_compose_people_args& a) { a.L_img = -1; }},
      {"L_img > L", [](pr_compose_people_args& a) { a.L_img = a.L + 1; }},
      {"null lines", [](pr_compose_people_args& a) { a.lines = nullptr; }},
      {"null text", [](pr_compose_people_args& a) { a.text = nullptr; }},
      {"null atlas", [](pr_compose_people_args& a) { a.atlas = nullptr; }},
      {"C 0", [](pr_compose_people_args& a) { a.C = 0; }},
      {"S 5", [](pr_compose_people_args& a) { a.S = PR_VIDEO_MAX_CLASSES + 1; }},
      {"CH 257", [](pr_compose_people_args& a) { a.CH = 257; }},
      {"CW 0", [](pr_compose_people_args& a) { a.CW = 0; }},
      {"adv 0", [](pr_compose_people_args& a) { a.adv[0] = 0; }},
      {"adv > CW", [](pr_compose_people_args& a) { a.adv[0] = a.CW + 1; }},
      {"ascent", [](pr_compose_people_args& a) { a.ascent[0] = 5000; }},
      {"N > n_frames without src_idx", [](pr_compose_people_args& a) { a.N = 2; }},
  };
  int failures = 0;
  for (const Bad& b : bad) {
    pr_compose_people_args a = ok;
    b.set(a);
    g_error[0] = 0;
    g_lds_asked = 0;
    const int rc = pr_compose_people(&a, nullptr);
    bool untouched = true;
    for (uint8_t v : out) untouched = untouched && v == 0xAB;
    if (rc != PR_ERR_INVALID || !untouched || g_lds_asked != 0 || !strstr(g_error, "pr_compose_people")) {
      fprintf(stderr, "%s: status %d, out %s, launched %d, message '%s'\n", b.what, rc, untouched ? "untouched" : "WRITTEN",
              g_lds_asked != 0, g_error);
      ++failures;
    }
  }
  if (pr_compose_people(nullptr, nullptr) != PR_ERR_INVALID) { fprintf(stderr, "null struct accepted\n"); ++failures; }
  pr_compose_people_args none = ok;
  none.N = 0; none.out = nullptr; none.frames = nullptr;
  if (pr_compose_people(&none, nullptr) != PR_OK) { fprintf(stderr, "N = 0 refused: %s\n", g_error); ++failures; }
  // ... and the valid call is valid: every byte written
  if (pr_compose_people(&ok, nullptr) != PR_OK) { fprintf(stderr, "the valid call was refused: %s\n", g_error); ++failures; }
  printf("compose_people_host: %d argument errors tried, %d failures\n", (int)(sizeof bad / sizeof bad[0]), failures);
  return failures ? 1 : 0;
}

int main(int argc, char** argv) {
  if (argc == 2 && !strcmp(argv[1], "--validate")) return validate();
  if (argc < 3) return 2;
  std::ifstream f(argv[1], std::ios::binary);
  int h[24];
  f.read((char*)h, sizeof h);
  pr_compose_people_args a{};
  a.N = h[0]; a.n_frames = h[1]; a.H = h[2]; a.W = h[3]; a.dst_h = h[4]; a.dst_w = h[5]; a.panel_w = h[6];
  a.K = h[7]; a.L = h[8]; a.L_img = h[9]; a.C = h[10]; a.S = h[11]; a.CH = h[12]; a.CW = h[13];
  for (int i = 0; i < 4; ++i) { a.adv[i] = h[14 + i]; a.ascent[i] = h[18 + i]; }
  // exact-size heap blocks: the sanitizer sees any byte read or written outside them
  std::vector<std::unique_ptr<uint8_t[]>> blocks;
  auto rd = [&](size_t n) {
    blocks.emplace_back(new uint8_t[n ? n : 1]);
    f.read((char*)blocks.back().get(), (std::streamsize)n);
    return blocks.back().get();
  };
  a.frames = rd((size_t)a.n_frames * a.H * a.W * 3);
  a.src_idx = (const int32_t*)rd((size_t)a.N * 4);
  if (!h[22]) a.src_idx = nullptr;
  a.box = (const int32_t*)rd((size_t)a.N * a.K * 16);
  a.box_rgb = rd((size_t)a.N * a.K * 4);
  if (!h[23]) a.box = nullptr;
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
  const int rc = pr_compose_people(&a, nullptr);
  if (rc != 0) fprintf(stderr, "%s\n", g_error);
  if (g_lds_asked > kLdsBytes) {
    fprintf(stderr, "the launch asked for %zu bytes of LDS\n", g_lds_asked);
    return 3;
  }
  for (int i = 0; i < shift; ++i)
    if (out[i] != 0xAB) { fprintf(stderr, "byte %d in front of out was written\n", i); return 4; }
  std::ofstream o(argv[2], std::ios::binary);
  o.write((char*)a.out, (std::streamsize)out_bytes);
  o.write((char*)status.data(), (std::streamsize)a.N * 4);
  printf("compose_people_host: status %d, %zu bytes of LDS\n", rc, g_lds_asked);
  return rc == 0 ? 0 : 1;
}
