// csrc/smooth.hip on the host (see host_shim.h): reads a case file, runs pr_smooth_tracks on exact-size heap blocks, writes
// the outputs.
//   case file: int32 N T m has_betas has_cam 0, f64 sigma, then track_start i32[T+1], frame_no i32[N], rotmat, betas, cam
//   usage: smooth_host <case> <out> <tile rows the tests assume>
//          smooth_host --validate      every argument error: PR_ERR_INVALID, the outputs untouched
#define HOST_SHIM_THREADS      // smooth.hip stages a tile in LDS and meets at barriers
#define NATIVE_QUIET_ERRORS    // --validate provokes every refusal and reads its message
#include "common.h"
#include "native_common.h"

using pr::g_error;
#include "smooth.hip"

#include <cmath>
#include <limits>

namespace {

struct Call {
  pr_smooth_params params{2, 0, 1.5};
  pr_smooth_inputs in{};
  pr_smooth_outputs out{};
  const int32_t* frame_no = nullptr;
  const int* track_start = nullptr;
  int T = 0, N = 0;
  int32_t* status = nullptr;
  void* workspace = nullptr;
  int run() const { return pr_smooth_tracks(&params, &in, frame_no, track_start, T, N, &out, status, workspace, nullptr); }
};

int validate() {
  const int N = 5, T = 2;
  std::vector<float> rot(N * 216, 0.f), betas(N * 10, 0.25f), cam(N * 3, 0.5f);
  for (int i = 0; i < N * 24; ++i) rot[i * 9] = rot[i * 9 + 4] = rot[i * 9 + 8] = 1.f;
  std::vector<int32_t> frame_no = {0, 1, 2, 0, 1};
  std::vector<int> start = {0, 3, 5};
  const size_t out_floats = (size_t)N * 229;
  std::vector<float> out(out_floats), ws(out_floats);
  std::vector<int32_t> status(N), replaced(N);
  auto fill = [&] {
    memset(out.data(), 0xAB, out_floats * 4);
    memset(ws.data(), 0xAB, out_floats * 4);
    memset(status.data(), 0xAB, N * 4);
    memset(replaced.data(), 0xAB, N * 4);
  };
  auto untouched = [&] {
    auto all = [](const void* p, size_t n) {
      for (size_t i = 0; i < n; ++i)
        if (((const uint8_t*)p)[i] != 0xAB) return false;
      return true;
    };
    return all(out.data(), out_floats * 4) && all(ws.data(), out_floats * 4) && all(status.data(), N * 4) && all(replaced.data(), N * 4);
  };
  Call ok;
  ok.in = {rot.data(), betas.data(), cam.data()};
  ok.out = {out.data(), out.data() + N * 216, out.data() + N * 226, replaced.data()};
  ok.frame_no = frame_no.data();
  ok.track_start = start.data();
  ok.T = T;
  ok.N = N;
  ok.status = status.data();
  ok.workspace = ws.data();
  static std::vector<int> bad_start;
  struct Bad {
    const char* what;
    void (*set)(Call&);
  };
  const Bad bad[] = {
      {"m -1", [](Call& c) { c.params.median_radius = -1; }},
      {"m 16", [](Call& c) { c.params.median_radius = 16; }},
      {"sigma < 0", [](Call& c) { c.params.sigma = -0.5; }},
      {"sigma nan", [](Call& c) { c.params.sigma = std::numeric_limits<double>::quiet_NaN(); }},
      {"sigma inf", [](Call& c) { c.params.sigma = std::numeric_limits<double>::infinity(); }},
      {"reserved", [](Call& c) { c.params.reserved = 1; }},
      {"N < 0", [](Call& c) { c.N = -1; }},
      {"T < 0", [](Call& c) { c.T = -1; }},
      {"null track_start", [](Call& c) { c.track_start = nullptr; }},
      {"start[0] != 0", [](Call& c) { bad_start = {1, 3, 5}; c.track_start = bad_start.data(); }},
      {"starts descend", [](Call& c) { bad_start = {0, 4, 3, 5}; c.track_start = bad_start.data(); c.T = 3; }},
      {"start[T] != N", [](Call& c) { bad_start = {0, 3, 4}; c.track_start = bad_start.data(); }},
      {"start[T] > N", [](Call& c) { bad_start = {0, 3, 6}; c.track_start = bad_start.data(); }},
      {"T = 0 with rows", [](Call& c) { c.T = 0; }},
      {"null rotmat in", [](Call& c) { c.in.rotmat = nullptr; }},
      {"null rotmat out", [](Call& c) { c.out.rotmat = nullptr; }},
      {"null frame_no", [](Call& c) { c.frame_no = nullptr; }},
      {"betas in only", [](Call& c) { c.out.betas = nullptr; }},
      {"betas out only", [](Call& c) { c.in.betas = nullptr; }},
      {"cam in only", [](Call& c) { c.out.cam = nullptr; }},
      {"cam out only", [](Call& c) { c.in.cam = nullptr; }},
      {"null workspace, both stages", [](Call& c) { c.workspace = nullptr; }},
      {"rotmat in place", [](Call& c) { c.out.rotmat = const_cast<float*>(c.in.rotmat); }},
      {"betas in place", [](Call& c) { c.out.betas = const_cast<float*>(c.in.betas); }},
      {"cam in place", [](Call& c) { c.out.cam = const_cast<float*>(c.in.cam); }},
      {"workspace = input", [](Call& c) { c.workspace = const_cast<float*>(c.in.rotmat); }},
      {"workspace = output", [](Call& c) { c.workspace = c.out.rotmat; }},
      {"status = frame_no", [](Call& c) { c.status = const_cast<int32_t*>(c.frame_no); }},
      {"status = replaced", [](Call& c) { c.status = c.out.replaced; }},
      {"cam out = betas out", [](Call& c) { c.out.cam = c.out.betas; }},
  };
  int failures = 0;
  for (const Bad& b : bad) {
    Call c = ok;
    b.set(c);
    g_error[0] = 0;
    fill();
    const int rc = c.run();
    if (rc != PR_ERR_INVALID || !untouched() || !strstr(g_error, "pr_smooth_tracks")) {
      fprintf(stderr, "%s: status %d, outputs %s, message '%s'\n", b.what, rc, untouched() ? "untouched" : "WRITTEN", g_error);
      ++failures;
    }
  }
  {
    Call c = ok;
    fill();
    if (pr_smooth_tracks(nullptr, &c.in, c.frame_no, c.track_start, T, N, &c.out, c.status, c.workspace, nullptr) != PR_ERR_INVALID ||
        pr_smooth_tracks(&c.params, nullptr, c.frame_no, c.track_start, T, N, &c.out, c.status, c.workspace, nullptr) != PR_ERR_INVALID ||
        pr_smooth_tracks(&c.params, &c.in, c.frame_no, c.track_start, T, N, nullptr, c.status, c.workspace, nullptr) != PR_ERR_INVALID ||
        !untouched()) {
      fprintf(stderr, "a null struct was accepted\n");
      ++failures;
    }
  }
  // N = 0 is valid, with or without tracks and without any tensor
  const int zero[] = {0, 0, 0};
  Call none;
  none.track_start = zero;
  none.T = 2;
  if (none.run() != PR_OK) { fprintf(stderr, "N = 0 refused: %s\n", g_error); ++failures; }
  none.T = 0;
  if (none.run() != PR_OK) { fprintf(stderr, "N = 0, T = 0 refused: %s\n", g_error); ++failures; }
  // ... and the valid call is valid, without status, replaced and (one stage) workspace too
  fill();
  if (ok.run() != PR_OK) { fprintf(stderr, "the valid call was refused: %s\n", g_error); ++failures; }
  for (int i = 0; i < N; ++i)
    if (status[i] != 0 || replaced[i] != 0) { fprintf(stderr, "status / replaced of row %d: %d / %d\n", i, status[i], replaced[i]); ++failures; }
  Call bare = ok;
  bare.status = nullptr;
  bare.out.replaced = nullptr;
  bare.workspace = nullptr;
  bare.params.sigma = 0.0;
  if (bare.run() != PR_OK) { fprintf(stderr, "the call without status, replaced and workspace was refused: %s\n", g_error); ++failures; }
  if (pr_smooth_workspace_bytes(-1, 1, 1) != 0 || pr_smooth_workspace_bytes(N, 1, 1) < out_floats * 4 ||
      pr_smooth_workspace_bytes(N, 0, 0) < (size_t)N * 216 * 4) {
    fprintf(stderr, "pr_smooth_workspace_bytes\n");
    ++failures;
  }
  printf("smooth_host: %d argument errors tried, %d failures\n", (int)(sizeof bad / sizeof bad[0]), failures);
  return failures ? 1 : 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc == 2 && !strcmp(argv[1], "--validate")) return validate();
  if (argc < 4) return 2;
  CHECK(pr_smooth_tile_rows() == atoi(argv[3]), "pr_smooth_tile_rows() = %d, the cases assume %s", pr_smooth_tile_rows(), argv[3]);
  std::ifstream f(argv[1], std::ios::binary);
  int32_t h[6];
  double sigma;
  f.read((char*)h, sizeof h);
  f.read((char*)&sigma, sizeof sigma);
  const int N = h[0], T = h[1];
  const bool has_betas = h[3], has_cam = h[4];
  // exact-size heap blocks: the sanitizer sees any byte read or written outside them
  auto rd = [&](auto& block, size_t n) { f.read((char*)block.get(), (std::streamsize)(n * sizeof block[0])); };
  auto start = exact<int32_t>(T + 1);
  auto frame_no = exact<int32_t>(N);
  auto rot = exact<float>((size_t)N * 216), betas = exact<float>((size_t)N * 10), cam = exact<float>((size_t)N * 3);
  rd(start, T + 1);
  rd(frame_no, N);
  rd(rot, (size_t)N * 216);
  if (has_betas) rd(betas, (size_t)N * 10);
  if (has_cam) rd(cam, (size_t)N * 3);
  CHECK((bool)f, "the case file is short");
  auto o_rot = exact<float>((size_t)N * 216), o_betas = exact<float>((size_t)N * 10), o_cam = exact<float>((size_t)N * 3);
  auto status = exact<int32_t>(N), replaced = exact<int32_t>(N);
  // the workspace holds exactly stage 1's outputs: not a float more than the tensors given
  auto ws = exact<float>((size_t)N * (216 + (has_betas ? 10 : 0) + (has_cam ? 3 : 0)));
  CHECK(pr_smooth_workspace_bytes(N, has_betas, has_cam) >= (size_t)N * (216 + (has_betas ? 10 : 0) + (has_cam ? 3 : 0)) * 4, "workspace size");
  std::vector<int> start_int(start.get(), start.get() + T + 1);
  Call c;
  c.params = {h[2], 0, sigma};
  c.in = {rot.get(), has_betas ? betas.get() : nullptr, has_cam ? cam.get() : nullptr};
  c.out = {o_rot.get(), has_betas ? o_betas.get() : nullptr, has_cam ? o_cam.get() : nullptr, replaced.get()};
  c.frame_no = frame_no.get();
  c.track_start = start_int.data();
  c.T = T;
  c.N = N;
  c.status = status.get();
  c.workspace = ws.get();
  const int rc = c.run();
  if (rc != 0) fprintf(stderr, "%s\n", g_error);
  std::ofstream o(argv[2], std::ios::binary);
  o.write((char*)o_rot.get(), (std::streamsize)N * 216 * 4);
  if (has_betas) o.write((char*)o_betas.get(), (std::streamsize)N * 10 * 4);
  if (has_cam) o.write((char*)o_cam.get(), (std::streamsize)N * 3 * 4);
  o.write((char*)status.get(), (std::streamsize)N * 4);
  o.write((char*)replaced.get(), (std::streamsize)N * 4);
  printf("smooth_host: status %d\n", rc);
  return rc == 0 && g_fail == 0 ? 0 : 1;
}
