// csrc/activity.hip on the host (see host_shim.h): reads a case file, runs pr_activity_tracks on exact-size heap blocks, writes
// the outputs.
//   case file: int32 N T H R G E, f64 dot_static dot_move dot_rapid, then track_start i32[T+1], frame_no i32[N], rotmat
//   usage: activity_host <case> <out> <tile rows the tests assume> <chunk rows>
//          activity_host --validate      every argument error: PR_ERR_INVALID, the outputs untouched
#define HOST_SHIM_THREADS      // activity.hip streams chunks through LDS and meets at barriers
#define NATIVE_QUIET_ERRORS    // --validate provokes every refusal and reads its message
#include "common.h"
#include "native_common.h"

using pr::g_error;
#include "activity.hip"

#include <cmath>
#include <limits>

namespace {

struct Call {
  pr_activity_params params{24, 3, 2, 3, 2.9, 2.8, 2.4};
  const float* rotmat = nullptr;
  const int32_t* frame_no = nullptr;
  const int* track_start = nullptr;
  int T = 0, N = 0;
  int32_t* flags = nullptr;
  int32_t* adds = nullptr;
  void* workspace = nullptr;
  int run() const { return pr_activity_tracks(&params, rotmat, frame_no, track_start, T, N, flags, adds, workspace, nullptr); }
};

int validate() {
  const int N = 5, T = 2;
  std::vector<float> rot(N * 216, 0.f);
  for (int i = 0; i < N * 24; ++i) rot[i * 9] = rot[i * 9 + 4] = rot[i * 9 + 8] = 1.f;
  std::vector<int32_t> frame_no = {0, 1, 2, 0, 1};
  std::vector<int> start = {0, 3, 5};
  std::vector<int32_t> flags(N * 4), adds(N * 4), ws(N * 3);
  auto fill = [&] {
    memset(flags.data(), 0xAB, flags.size() * 4);
    memset(adds.data(), 0xAB, adds.size() * 4);
    memset(ws.data(), 0xAB, ws.size() * 4);
  };
  auto untouched = [&] {
    auto all = [](const std::vector<int32_t>& v) {
      for (size_t i = 0; i < v.size() * 4; ++i)
        if (((const uint8_t*)v.data())[i] != 0xAB) return false;
      return true;
    };
    return all(flags) && all(adds) && all(ws);
  };
  Call ok;
  ok.rotmat = rot.data();
  ok.frame_no = frame_no.data();
  ok.track_start = start.data();
  ok.T = T;
  ok.N = N;
  ok.flags = flags.data();
  ok.adds = adds.data();
  ok.workspace = ws.data();
  static std::vector<int> bad_start;
  struct Bad {
    const char* what;
    void (*set)(Call&);
  };
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  static double s_nan, s_inf;
  s_nan = nan;
  s_inf = inf;
  const Bad bad[] = {
      {"H 0", [](Call& c) { c.params.hold_frames = 0; }},
      {"H 16385", [](Call& c) { c.params.hold_frames = 16385; }},
      {"R 0", [](Call& c) { c.params.rapid_frames = 0; }},
      {"R > H", [](Call& c) { c.params.rapid_frames = 25; }},
      {"G 0", [](Call& c) { c.params.gap_frames = 0; }},
      {"E -1", [](Call& c) { c.params.rep_events = -1; }},
      {"static nan", [](Call& c) { c.params.dot_static = s_nan; }},
      {"static > 3", [](Call& c) { c.params.dot_static = 3.5; }},
      {"move inf", [](Call& c) { c.params.dot_move = s_inf; }},
      {"move < -1", [](Call& c) { c.params.dot_move = -1.5; }},
      {"rapid nan", [](Call& c) { c.params.dot_rapid = s_nan; }},
      {"rapid -inf", [](Call& c) { c.params.dot_rapid = -s_inf; }},
      {"N < 0", [](Call& c) { c.N = -1; }},
      {"T < 0", [](Call& c) { c.T = -1; }},
      {"null track_start", [](Call& c) { c.track_start = nullptr; }},
      {"start[0] != 0", [](Call& c) { bad_start = {1, 3, 5}; c.track_start = bad_start.data(); }},
      {"starts descend", [](Call& c) { bad_start = {0, 4, 3, 5}; c.track_start = bad_start.data(); c.T = 3; }},
      {"start[T] != N", [](Call& c) { bad_start = {0, 3, 4}; c.track_start = bad_start.data(); }},
      {"start[T] > N", [](Call& c) { bad_start = {0, 3, 6}; c.track_start = bad_start.data(); }},
      {"T = 0 with rows", [](Call& c) { c.T = 0; }},
      {"null rotmat", [](Call& c) { c.rotmat = nullptr; }},
      {"null frame_no", [](Call& c) { c.frame_no = nullptr; }},
      {"null flags", [](Call& c) { c.flags = nullptr; }},
      {"null adds", [](Call& c) { c.adds = nullptr; }},
      {"null workspace", [](Call& c) { c.workspace = nullptr; }},
      {"workspace misaligned", [](Call& c) { c.workspace = (char*)c.workspace + 2; }},
      {"flags = adds", [](Call& c) { c.adds = c.flags; }},
      {"flags = frame_no", [](Call& c) { c.flags = const_cast<int32_t*>(c.frame_no); }},
      {"workspace = rotmat", [](Call& c) { c.workspace = const_cast<float*>(c.rotmat); }},
      {"workspace = adds", [](Call& c) { c.workspace = c.adds; }},
  };
  int failures = 0;
  for (const Bad& b : bad) {
    Call c = ok;
    b.set(c);
    g_error[0] = 0;
    fill();
    const int rc = c.run();
    if (rc != PR_ERR_INVALID || !untouched() || !strstr(g_error, "pr_activity_tracks")) {
      fprintf(stderr, "%s: status %d, outputs %s, message '%s'\n", b.what, rc, untouched() ? "untouched" : "WRITTEN", g_error);
      ++failures;
    }
  }
  fill();
  if (pr_activity_tracks(nullptr, ok.rotmat, ok.frame_no, ok.track_start, T, N, ok.flags, ok.adds, ok.workspace, nullptr) != PR_ERR_INVALID ||
      !untouched()) {
    fprintf(stderr, "null params were accepted\n");
    ++failures;
  }
  // N = 0 is valid, with or without tracks and without any tensor
  const int zero[] = {0, 0, 0};
  Call none;
  none.track_start = zero;
  none.T = 2;
  if (none.run() != PR_OK) { fprintf(stderr, "N = 0 refused: %s\n", g_error); ++failures; }
  none.T = 0;
  if (none.run() != PR_OK) { fprintf(stderr, "N = 0, T = 0 refused: %s\n", g_error); ++failures; }
  // ... and the valid call is valid: five identical rows, tracks too short to be covered
  fill();
  if (ok.run() != PR_OK) { fprintf(stderr, "the valid call was refused: %s\n", g_error); ++failures; }
  for (int i = 0; i < N * 4; ++i)
    if (flags[i] != 0 || adds[i] != 0) { fprintf(stderr, "flags / adds [%d]: %d / %d\n", i, flags[i], adds[i]); ++failures; }
  if (pr_activity_workspace_bytes(-1) != 0 || pr_activity_workspace_bytes(N) < (size_t)N * 12 || pr_activity_workspace_bytes(N) % 256) {
    fprintf(stderr, "pr_activity_workspace_bytes\n");
    ++failures;
  }
  printf("activity_host: %d argument errors tried, %d failures\n", (int)(sizeof bad / sizeof bad[0]), failures);
  return failures ? 1 : 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc == 2 && !strcmp(argv[1], "--validate")) return validate();
  if (argc < 5) return 2;
  CHECK(pr_activity_tile_rows() == atoi(argv[3]), "pr_activity_tile_rows() = %d, the cases assume %s", pr_activity_tile_rows(), argv[3]);
  CHECK(pr_activity_chunk_rows() == atoi(argv[4]), "pr_activity_chunk_rows() = %d, the cases assume %s", pr_activity_chunk_rows(), argv[4]);
  std::ifstream f(argv[1], std::ios::binary);
  int32_t h[6];
  double dot[3];
  f.read((char*)h, sizeof h);
  f.read((char*)dot, sizeof dot);
  const int N = h[0], T = h[1];
  // exact-size heap blocks: the sanitizer sees any byte read or written outside them
  auto rd = [&](auto& block, size_t n) { f.read((char*)block.get(), (std::streamsize)(n * sizeof block[0])); };
  auto start = exact<int32_t>(T + 1);
  auto frame_no = exact<int32_t>(N);
  auto rot = exact<float>((size_t)N * 216);
  rd(start, T + 1);
  rd(frame_no, N);
  rd(rot, (size_t)N * 216);
  CHECK((bool)f, "the case file is short");
  auto flags = exact<int32_t>((size_t)N * 4), adds = exact<int32_t>((size_t)N * 4);
  auto ws = exact<int32_t>((size_t)N * 3);           // exactly the three masks, not the rounded size
  CHECK(pr_activity_workspace_bytes(N) >= (size_t)N * 12, "workspace size");
  std::vector<int> start_int(start.get(), start.get() + T + 1);
  Call c;
  c.params = {h[2], h[3], h[4], h[5], dot[0], dot[1], dot[2]};
  c.rotmat = rot.get();
  c.frame_no = frame_no.get();
  c.track_start = start_int.data();
  c.T = T;
  c.N = N;
  c.flags = flags.get();
  c.adds = adds.get();
  c.workspace = ws.get();
  const int rc = c.run();
  if (rc != 0) fprintf(stderr, "%s\n", g_error);
  std::ofstream o(argv[2], std::ios::binary);
  o.write((char*)flags.get(), (std::streamsize)N * 16);
  o.write((char*)adds.get(), (std::streamsize)N * 16);
  printf("activity_host: status %d\n", rc);
  return rc == 0 && g_fail == 0 ? 0 : 1;
}
