// Device-free half of the person detector (include/poserisk_hip.h, section j8): the fixed topology of darknet's yolov3.cfg as
// a table, where each convolution's parameters lie in the darknet weight file and in the packed blob the kernels read,
// BatchNorm folding in float64, and the activation-buffer plan of the handle (det.hip).  No device call and no HIP header:
// tests/test_detector_native.py builds this file with g++ under sanitizers.
#include "det_host.h"

#include <climits>
#include <cmath>

namespace pr {
namespace {

int round_up(int v, int m) { return (v + m - 1) / m * m; }

struct Builder {
  std::vector<pr_det_layer> L;
  int64_t w_off = 0, p_off = 0;

  pr_det_layer blank(int type) {
    pr_det_layer l;
    memset(&l, 0, sizeof l);
    l.type = type;
    l.from0 = l.from1 = -1;
    l.weight_offset = l.pack_offset = -1;
    if (!L.empty()) l.cin = L.back().cout, l.down = L.back().down;
    else l.cin = 3, l.down = 1;
    l.cout = l.cin;
    return l;
  }
  void conv(int filters, int k, int stride, int bn = 1) {
    pr_det_layer l = blank(PR_DET_CONV);
    l.cout = filters, l.ksize = k, l.stride = stride, l.bn = bn;
    l.down *= stride;
    l.cin_pad = round_up(l.cin, 4);
    l.cout_pad = round_up(filters, kDetCoutTile);
    l.kpad = round_up(k * k * l.cin_pad, kDetKTile);
    l.weight_offset = w_off;
    l.pack_offset = p_off;
    w_off += (int64_t)filters * (bn ? 4 : 1) + (int64_t)filters * l.cin * k * k;
    p_off += (int64_t)l.cout_pad + (int64_t)l.cout_pad * l.kpad;
    L.push_back(l);
  }
  void shortcut() {
    pr_det_layer l = blank(PR_DET_SHORTCUT);
    l.from0 = (int)L.size() - 3;
    L.push_back(l);
  }
  void block(int planes, int n) {   // n x (1x1 to planes / 2, 3x3 to planes, shortcut)
    for (int i = 0; i < n; ++i) conv(planes / 2, 1, 1), conv(planes, 3, 1), shortcut();
  }
  void route(int a, int b = -1) {
    pr_det_layer l = blank(PR_DET_ROUTE);
    l.from0 = a, l.from1 = b;
    l.cin = l.cout = L[a].cout + (b >= 0 ? L[b].cout : 0);
    l.down = L[a].down;
    L.push_back(l);
  }
  void upsample() {
    pr_det_layer l = blank(PR_DET_UPSAMPLE);
    l.stride = 2;
    l.down /= 2;
    L.push_back(l);
  }
  void yolo() { L.push_back(blank(PR_DET_YOLO)); }
  void neck(int planes) {           // the five alternating convolutions, the 3x3 in front of the head, the head, yolo
    for (int i = 0; i < 3; ++i) conv(planes, 1, 1), conv(2 * planes, 3, 1);
    conv(kDetHeadChannels, 1, 1, 0);
    yolo();
  }
};

const std::vector<pr_det_layer>& full_table() {
  static const std::vector<pr_det_layer> table = [] {
    Builder b;
    b.conv(32, 3, 1);
    b.conv(64, 3, 2), b.block(64, 1);
    b.conv(128, 3, 2), b.block(128, 2);
    b.conv(256, 3, 2), b.block(256, 8);      // ends at layer 36
    b.conv(512, 3, 2), b.block(512, 8);      // ends at layer 61
    b.conv(1024, 3, 2), b.block(1024, 4);    // ends at layer 74
    b.neck(512);                             // 75..82
    b.route((int)b.L.size() - 4), b.conv(256, 1, 1), b.upsample(), b.route((int)b.L.size() - 1, 61);
    b.neck(256);                             // 87..94
    b.route((int)b.L.size() - 4), b.conv(128, 1, 1), b.upsample(), b.route((int)b.L.size() - 1, 36);
    b.neck(128);                             // 99..106
    return b.L;
  }();
  return table;
}

bool det_n_ok(int n) { return n >= 1 && n <= kDetLayers; }

// One convolution folded in float64: bias[o] = b', put(o * kpad + tap * cin_pad + ci, w') for every weight (OIHW in the body)
template <typename Put>
void fold_conv(const pr_det_layer& c, const float* src, double bn_eps, float* bias, Put put) {
  const float* wsrc = src + (size_t)c.cout * (c.bn ? 4 : 1);
  const int kk = c.ksize * c.ksize;
  for (int o = 0; o < c.cout; ++o) {
    double scale = 1.0, shift = src[o];                              // head: bias, weights as they are
    if (c.bn) {                                                      // darknet order: beta, gamma, mean, var
      const double beta = src[o], gamma = src[c.cout + o], mean = src[2 * c.cout + o], var = src[3 * c.cout + o];
      scale = gamma / std::sqrt(var + bn_eps);
      shift = beta - mean * scale;
    }
    bias[o] = (float)shift;
    for (int ci = 0; ci < c.cin; ++ci)
      for (int t2 = 0; t2 < kk; ++t2)
        put((size_t)o * c.kpad + (size_t)t2 * c.cin_pad + ci, (float)(wsrc[((size_t)o * c.cin + ci) * kk + t2] * scale));
  }
}

}  // namespace

void det_topology(int n_layers, std::vector<pr_det_layer>* out) {
  const auto& t = full_table();
  out->assign(t.begin(), t.begin() + n_layers);
}

void det_pack_offsets_bf16(int n_layers, std::vector<int64_t>* out) {
  const auto& t = full_table();
  out->assign(n_layers, -1);
  int64_t off = 0;
  for (int l = 0; l < n_layers; ++l) {
    if (t[l].type != PR_DET_CONV) continue;
    (*out)[l] = off;                                      // layer 0 keeps fp32 weights: it runs on the fp32 MFMA
    off += (int64_t)t[l].cout_pad * 4 + (int64_t)t[l].cout_pad * t[l].kpad * (l == 0 ? 4 : 2);
  }
}

int det_plan(int S_h, int S_w, DetPlan* plan, int precision) {
  PR_REQUIRE(precision == 0 || precision == 1, "detector: precision = %d, must be 0 (fp32) or 1 (bf16)", precision);
  PR_REQUIRE(S_h >= 32 && S_w >= 32 && S_h % 32 == 0 && S_w % 32 == 0 && S_h <= 4096 && S_w <= 4096,
             "detector: the network input %d x %d (S_w x S_h) must be multiples of 32 in 32..4096", S_w, S_h);
  det_topology(kDetLayers, &plan->layers);
  const auto& L = plan->layers;
  const int n = (int)L.size();
  // store[l]: the layer whose buffer holds l's output -- a view's is its source's, a shortcut's the convolution's in front
  std::vector<int> store(n), last(n, -1);
  for (int l = 0; l < n; ++l) {
    store[l] = l;
    if (L[l].type == PR_DET_YOLO || L[l].type == PR_DET_SHORTCUT) store[l] = store[l - 1];
    if (L[l].type == PR_DET_ROUTE && L[l].from1 < 0) store[l] = store[L[l].from0];
  }
  auto reads = [&](int l, int src) { last[store[src]] = std::max(last[store[src]], l); };
  for (int l = 0; l < n; ++l) {
    const int t = L[l].type;
    if ((t == PR_DET_CONV && l > 0) || t == PR_DET_UPSAMPLE) reads(l, l - 1);
    if (t == PR_DET_SHORTCUT) reads(l, L[l].from0);
    if (t == PR_DET_ROUTE && L[l].from1 >= 0) {
      reads(l, L[l].from0), reads(l, L[l].from1);
      // upsample-into-concat (det.hip): the route's kernel reads the upsample's INPUT, which must outlive the upsample
      if (L[L[l].from0].type == PR_DET_UPSAMPLE) reads(l, L[l].from0 - 1);
    }
    if (t == PR_DET_YOLO) last[store[l]] = INT_MAX;     // a head tensor is an output: kept to the end
  }
  plan->slot.assign(n, -1);
  plan->gh.resize(n), plan->gw.resize(n);
  plan->slot_floats.clear();
  plan->slot_frame_bytes.clear();
  plan->elem_bytes.assign(n, precision == 1 ? 2 : 4);
  for (int l = 0; l < n; ++l)      // a head convolution writes fp32 in either precision; the yolo layer behind it is its view
    if (L[l].type == PR_DET_YOLO) plan->elem_bytes[l] = plan->elem_bytes[l - 1] = 4;
  std::vector<char> busy;
  for (int l = 0; l < n; ++l) {
    plan->gh[l] = S_h / L[l].down, plan->gw[l] = S_w / L[l].down;
    const size_t floats = (size_t)plan->gh[l] * plan->gw[l] * L[l].cout;
    if (store[l] != l) {
      plan->slot[l] = plan->slot[store[l]];
    } else {                                            // the output's buffer is taken BEFORE the inputs' are released
      size_t s = 0;
      while (s < busy.size() && busy[s]) ++s;
      if (s == busy.size()) busy.push_back(0), plan->slot_floats.push_back(0), plan->slot_frame_bytes.push_back(0);
      busy[s] = 1;
      plan->slot[l] = (int)s;
      plan->slot_floats[s] = std::max(plan->slot_floats[s], floats);
      plan->slot_frame_bytes[s] = std::max(plan->slot_frame_bytes[s], floats * plan->elem_bytes[l]);
    }
    for (int t = 0; t <= l; ++t)
      if (store[t] == t && last[t] == l) busy[plan->slot[t]] = 0;
  }
  return PR_OK;
}

}  // namespace pr

extern "C" {

int pr_det_topology(int n_layers, pr_det_layer* layers_host) {
  using namespace pr;
  PR_REQUIRE(det_n_ok(n_layers), "pr_det_topology: n_layers = %d, must lie in 1..%d", n_layers, kDetLayers);
  PR_REQUIRE(layers_host, "pr_det_topology: null layers_host");
  std::vector<pr_det_layer> t;
  det_topology(n_layers, &t);
  memcpy(layers_host, t.data(), t.size() * sizeof(pr_det_layer));
  return PR_OK;
}

size_t pr_det_weight_floats(int n_layers) {
  using namespace pr;
  if (!det_n_ok(n_layers)) return 0;
  size_t n = 0;
  const auto& t = full_table();
  for (int l = 0; l < n_layers; ++l)
    if (t[l].type == PR_DET_CONV) n += (size_t)t[l].cout * (t[l].bn ? 4 : 1) + (size_t)t[l].cout * t[l].cin * t[l].ksize * t[l].ksize;
  return n;
}

size_t pr_det_packed_floats(int n_layers) {
  using namespace pr;
  if (!det_n_ok(n_layers)) return 0;
  size_t n = 0;
  const auto& t = full_table();
  for (int l = 0; l < n_layers; ++l)
    if (t[l].type == PR_DET_CONV) n += (size_t)t[l].cout_pad * (1 + t[l].kpad);
  return n;
}

int pr_det_fold_pack(int n_layers, const float* weights_host, size_t n_floats, double bn_eps, float* packed_host, size_t packed_floats) {
  using namespace pr;
  PR_REQUIRE(det_n_ok(n_layers), "pr_det_fold_pack: n_layers = %d, must lie in 1..%d", n_layers, kDetLayers);
  PR_REQUIRE(weights_host, "pr_det_fold_pack: null weights_host");
  PR_REQUIRE(packed_host, "pr_det_fold_pack: null packed_host");
  PR_REQUIRE(n_floats == pr_det_weight_floats(n_layers), "pr_det_fold_pack: n_floats = %zu, but the first %d layers hold %zu", n_floats,
             n_layers, pr_det_weight_floats(n_layers));
  PR_REQUIRE(packed_floats == pr_det_packed_floats(n_layers), "pr_det_fold_pack: packed_floats = %zu, but the first %d layers pack to %zu",
             packed_floats, n_layers, pr_det_packed_floats(n_layers));
  PR_REQUIRE(bn_eps > 0 && bn_eps < 1, "pr_det_fold_pack: bn_eps = %g, must lie in (0, 1)", bn_eps);
  memset(packed_host, 0, packed_floats * sizeof(float));
  const auto& t = full_table();
  for (int l = 0; l < n_layers; ++l) {
    const pr_det_layer& c = t[l];
    if (c.type != PR_DET_CONV) continue;
    float* bias = packed_host + c.pack_offset;
    float* w = bias + c.cout_pad;
    fold_conv(c, weights_host + c.weight_offset, bn_eps, bias, [&](size_t i, float v) { w[i] = v; });
  }
  return PR_OK;
}

size_t pr_det_packed_bytes_bf16(int n_layers) {
  using namespace pr;
  if (!det_n_ok(n_layers)) return 0;
  size_t n = 0;
  const auto& t = full_table();
  for (int l = 0; l < n_layers; ++l)
    if (t[l].type == PR_DET_CONV) n += (size_t)t[l].cout_pad * 4 + (size_t)t[l].cout_pad * t[l].kpad * (l == 0 ? 4 : 2);
  return n;
}

int pr_det_fold_pack_bf16(int n_layers, const float* weights_host, size_t n_floats, double bn_eps, void* packed_host, size_t packed_bytes) {
  using namespace pr;
  PR_REQUIRE(det_n_ok(n_layers), "pr_det_fold_pack_bf16: n_layers = %d, must lie in 1..%d", n_layers, kDetLayers);
  PR_REQUIRE(weights_host, "pr_det_fold_pack_bf16: null weights_host");
  PR_REQUIRE(packed_host, "pr_det_fold_pack_bf16: null packed_host");
  PR_REQUIRE(n_floats == pr_det_weight_floats(n_layers), "pr_det_fold_pack_bf16: n_floats = %zu, but the first %d layers hold %zu", n_floats,
             n_layers, pr_det_weight_floats(n_layers));
  PR_REQUIRE(packed_bytes == pr_det_packed_bytes_bf16(n_layers),
             "pr_det_fold_pack_bf16: packed_bytes = %zu, but the first %d layers pack to %zu", packed_bytes, n_layers,
             pr_det_packed_bytes_bf16(n_layers));
  PR_REQUIRE(bn_eps > 0 && bn_eps < 1, "pr_det_fold_pack_bf16: bn_eps = %g, must lie in (0, 1)", bn_eps);
  memset(packed_host, 0, packed_bytes);
  const auto& t = full_table();
  std::vector<int64_t> off;
  det_pack_offsets_bf16(n_layers, &off);
  std::vector<float> bias;
  for (int l = 0; l < n_layers; ++l) {
    const pr_det_layer& c = t[l];
    if (c.type != PR_DET_CONV) continue;
    char* base = static_cast<char*>(packed_host) + off[l];       // memcpy throughout: packed_host is only byte-aligned for us
    char* w = base + (size_t)c.cout_pad * 4;
    bias.assign(c.cout_pad, 0.f);
    if (l == 0) {
      fold_conv(c, weights_host + c.weight_offset, bn_eps, bias.data(), [&](size_t i, float v) { memcpy(w + 4 * i, &v, 4); });
    } else {
      fold_conv(c, weights_host + c.weight_offset, bn_eps, bias.data(), [&](size_t i, float v) {
        const uint16_t r = bf16_rne(v);
        memcpy(w + 2 * i, &r, 2);
      });
    }
    memcpy(base, bias.data(), (size_t)c.cout_pad * 4);
  }
  return PR_OK;
}

}  // extern "C"
