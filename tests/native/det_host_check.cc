// The device-free half of the person detector (csrc/det_host.cc) as a stand-alone program, for a build under
// ASan + UBSan (tests/test_detector_native.py): the topology table, fold + pack of a TRUNCATED table into an
// exact-size heap block, the refusals, and the activation-buffer plan checked structurally at several input sizes.
//   det_host_check <n_layers> <weights.f32> <bn_eps> <packed_out.f32>
#include <string>

#define NATIVE_QUIET_ERRORS    // the refusals are provoked on purpose and their messages read
#include "native_common.h"
#include "det_host.h"

// Walks the plan as det.hip does and checks that no step writes a buffer it reads, and that every buffer a step reads still
// holds the tensor it wants (symbolic: content[slot] = the layer whose output is there).
static void check_plan(int S_h, int S_w) {
  pr::DetPlan P;
  CHECK(pr::det_plan(S_h, S_w, &P) == PR_OK, "det_plan(%d, %d): %s", S_h, S_w, pr::g_error);
  const auto& L = P.layers;
  const int n = (int)L.size();
  std::vector<int> content(P.slot_floats.size(), -1);
  auto holds = [&](int layer) {      // the layer whose tensor a read of `layer` wants: views resolve to their source
    int l = layer;
    while (L[l].type == PR_DET_YOLO || (L[l].type == PR_DET_ROUTE && L[l].from1 < 0)) l = L[l].type == PR_DET_YOLO ? l - 1 : L[l].from0;
    return l;
  };
  auto want = [&](int step, int layer) {
    const int src = holds(layer);
    CHECK(content[P.slot[src]] == src, "%dx%d: layer %d reads layer %d, but its buffer %d holds layer %d", S_h, S_w, step, src, P.slot[src],
          content[P.slot[src]]);
    return P.slot[src];
  };
  for (int l = 0; l < n; ++l) {
    const size_t floats = (size_t)P.gh[l] * P.gw[l] * L[l].cout;
    CHECK(P.gh[l] == S_h / L[l].down && P.gw[l] == S_w / L[l].down, "grid of layer %d", l);
    CHECK(P.slot[l] >= 0 && P.slot_floats[P.slot[l]] >= floats, "%dx%d: layer %d does not fit its buffer", S_h, S_w, l);
    if (L[l].type == PR_DET_CONV) {
      const bool fused = l + 1 < n && L[l + 1].type == PR_DET_SHORTCUT;
      const int x = l ? want(l, l - 1) : -1, r = fused ? want(l, L[l + 1].from0) : -1;
      CHECK(P.slot[l] != x && P.slot[l] != r, "%dx%d: convolution %d writes a buffer it reads", S_h, S_w, l);
      if (fused) CHECK(P.slot[l + 1] == P.slot[l], "shortcut %d is not in its convolution's buffer", l + 1);
      content[P.slot[l]] = fused ? l + 1 : l;
      if (fused) ++l;
    } else if (L[l].type == PR_DET_UPSAMPLE) {
      CHECK(P.slot[l] != want(l, l - 1), "upsample %d in place", l);
      content[P.slot[l]] = l;
      // upsample-into-concat: the route behind it is filled by one kernel that reads the upsample's input
      if (l + 1 < n && L[l + 1].type == PR_DET_ROUTE && L[l + 1].from0 == l && L[l + 1].from1 >= 0)
        CHECK(P.slot[l + 1] != P.slot[holds(l - 1)], "%dx%d: route %d is written over the input of upsample %d", S_h, S_w, l + 1, l);
    } else if (L[l].type == PR_DET_ROUTE && L[l].from1 >= 0) {
      const int a = want(l, L[l].from0), b = want(l, L[l].from1);
      CHECK(P.slot[l] != a && P.slot[l] != b, "route %d in place", l);
      content[P.slot[l]] = l;
    } else {
      CHECK(L[l].type != PR_DET_SHORTCUT, "a shortcut at %d without a convolution in front", l);
      CHECK(P.slot[l] == P.slot[holds(l)], "view %d is not in its source's buffer", l);
    }
  }
  const int heads[3] = {81, 93, 105};
  for (int h : heads) CHECK(content[P.slot[h]] == h, "%dx%d: head %d was overwritten before the end", S_h, S_w, h);
}

int main(int argc, char** argv) {
  if (argc != 5) return 2;
  const int n_layers = atoi(argv[1]);
  const double eps = atof(argv[3]);
  std::vector<pr_det_layer> table(PR_DET_NUM_LAYERS);
  CHECK(pr_det_topology(PR_DET_NUM_LAYERS, table.data()) == PR_OK, "topology");
  int convs = 0, shortcuts = 0;
  for (const auto& l : table) convs += l.type == PR_DET_CONV, shortcuts += l.type == PR_DET_SHORTCUT;
  CHECK(convs == 75 && shortcuts == 23, "75 convolutions and 23 shortcuts, got %d and %d", convs, shortcuts);
  CHECK(pr_det_weight_floats(PR_DET_NUM_LAYERS) == 62001757u, "62001757 floats, got %zu", pr_det_weight_floats(PR_DET_NUM_LAYERS));
  CHECK(pr_det_topology(0, table.data()) == PR_ERR_INVALID && pr_det_topology(108, table.data()) == PR_ERR_INVALID, "n_layers refused");
  CHECK(pr_det_topology(3, nullptr) == PR_ERR_INVALID, "null table refused");
  CHECK(pr_det_weight_floats(0) == 0 && pr_det_packed_floats(108) == 0, "counts outside 1..107");

  // exact-size heap blocks: a read or write one float off is the sanitizer's
  const size_t nw = pr_det_weight_floats(n_layers), np_ = pr_det_packed_floats(n_layers);
  std::vector<float> w(nw), packed(np_);
  FILE* f = fopen(argv[2], "rb");
  if (!f || fread(w.data(), sizeof(float), nw, f) != nw) return 3;
  fclose(f);
  CHECK(pr_det_fold_pack(n_layers, w.data(), nw, eps, packed.data(), np_) == PR_OK, "fold_pack: %s", pr::g_error);
  CHECK(pr_det_fold_pack(n_layers, w.data(), nw - 1, eps, packed.data(), np_) == PR_ERR_INVALID, "a short body refused");
  CHECK(pr_det_fold_pack(n_layers, w.data(), nw, eps, packed.data(), np_ + 1) == PR_ERR_INVALID, "a wrong capacity refused");
  CHECK(pr_det_fold_pack(n_layers, w.data(), nw, 0.0, packed.data(), np_) == PR_ERR_INVALID, "bn_eps = 0 refused");
  CHECK(pr_det_fold_pack(n_layers, nullptr, nw, eps, packed.data(), np_) == PR_ERR_INVALID, "null weights refused");
  f = fopen(argv[4], "wb");
  if (!f || fwrite(packed.data(), sizeof(float), np_, f) != np_) return 4;
  fclose(f);

  const int sizes[][2] = {{32, 32}, {32, 64}, {64, 96}, {256, 416}, {416, 416}, {608, 608}};
  for (const auto& s : sizes) check_plan(s[0], s[1]);
  pr::DetPlan P;
  CHECK(pr::det_plan(48, 64, &P) == PR_ERR_INVALID && pr::det_plan(0, 64, &P) == PR_ERR_INVALID, "bad sizes refused");
  printf("det_host_check: %zu floats packed to %zu, %d failures\n", nw, np_, g_fail);
  return g_fail ? 1 : 0;
}
