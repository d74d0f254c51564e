// Device-free half of pr_hmr_create (see host_plan.h): blob layout, BatchNorm folding, weight packing, the launch plan.
// Each whole layout is packed in ONE place -- conv_pack_side_by_side, bottleneck_pack_bf16 -- which the plan (build) and the
// stand-alone test entries (capi.hip) both call, so the kernels' own tests and the encoder read the same definition.
// Compiled into libposerisk_hip.so by hipcc as plain C++ and, for tests/native/host_plan_check.cc, by g++ with
// -fsanitize=address,undefined.  No HIP header may be included here.
#include "host_plan.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <utility>
#include <vector>

namespace pr {

// ---- weight packing -------------------------------------------------------------------------------------------------
int conv_kpad_bf16(int K) { return ceil_div(K, 64) * 64; }

unsigned short f32_to_bf16_host(float f) {  // round-to-nearest-even; NaN stays NaN
  unsigned u;
  memcpy(&u, &f, 4);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (unsigned short)((u >> 16) | 0x40);
  return (unsigned short)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}

void conv_pack_weights_bf16(const float* w, const double* scale, int Cout, int Cin_real, int cin_pad, int KH,
                            int KW, unsigned short* out) {
  const int Kpad = conv_kpad_bf16(KH * KW * cin_pad);
  for (int o = 0; o < Cout; ++o) {
    unsigned short* row = out + (size_t)o * Kpad;
    for (int k = 0; k < Kpad; ++k) row[k] = 0;
    const double s = scale ? scale[o] : 1.0;
    for (int ci = 0; ci < Cin_real; ++ci)
      for (int kh = 0; kh < KH; ++kh)
        for (int kw = 0; kw < KW; ++kw)
          row[conv_k_index_bf16(kh * KW + kw, ci, KH * KW, cin_pad)] =
              f32_to_bf16_host((float)((double)w[(((size_t)o * Cin_real + ci) * KH + kh) * KW + kw] * s));
  }
}

void conv_pack_weights(const float* w, const double* scale, int Cout, int Cin_real, int cin_pad,
                       int KH, int KW, float* out) {
  const int K = KH * KW * cin_pad;
  const int Kpad = ceil_div(K, kConvBK) * kConvBK;
  for (int o = 0; o < Cout; ++o) {
    float* row = out + (size_t)o * Kpad;
    for (int k = 0; k < Kpad; ++k) row[k] = 0.f;
    const double s = scale ? scale[o] : 1.0;
    for (int ci = 0; ci < Cin_real; ++ci)
      for (int kh = 0; kh < KH; ++kh)
        for (int kw = 0; kw < KW; ++kw) {
          const double v = (double)w[(((size_t)o * Cin_real + ci) * KH + kh) * KW + kw] * s;
          row[(kh * KW + kw) * cin_pad + ci] = (float)v;
        }
  }
}

void conv_winograd_pack_weights(const float* w, const double* scale, int Cout, int Cin, int form, float* out) {
  // U = G g G^T in double, one rounding to fp32;  layout [(m+2)^2][Cout][Cin]
  static const double G2[4][3] = {{1, 0, 0}, {0.5, 0.5, 0.5}, {0.5, -0.5, 0.5}, {0, 0, 1}};
  static const double G4[6][3] = {{1.0 / 4, 0, 0},          {-1.0 / 6, -1.0 / 6, -1.0 / 6}, {-1.0 / 6, 1.0 / 6, -1.0 / 6},
                                  {1.0 / 24, 1.0 / 12, 1.0 / 6}, {1.0 / 24, -1.0 / 12, 1.0 / 6},  {0, 0, 1}};
  // form 5: G[j] = [1, p_j, p_j^2] / N_j on the points 0, +-a, +-b (N_0 = a^2 b^2, N_a = 2 a^2 (a^2 - b^2),
  // N_b = 2 b^2 (b^2 - a^2)), last row [0, 0, 1]; with a = 1, b = 2 these are G4's rows
  double G5[6][3];
  {
    const double a = kWa, b = kWb, a2 = a * a, b2 = b * b, Na = 2 * a2 * (a2 - b2), Nb = 2 * b2 * (b2 - a2);
    const double rows[6][3] = {{1 / (a2 * b2), 0, 0}, {1 / Na, a / Na, a2 / Na}, {1 / Na, -a / Na, a2 / Na},
                               {1 / Nb, b / Nb, b2 / Nb}, {1 / Nb, -b / Nb, b2 / Nb}, {0, 0, 1}};
    for (int i = 0; i < 6; ++i)
      for (int j = 0; j < 3; ++j) G5[i][j] = rows[i][j];
  }
  const int m = conv_winograd_tile(form);
  const int n = m + 2;
  const double(*G)[3] = form == 5 ? G5 : m == 4 ? G4 : G2;
  for (int o = 0; o < Cout; ++o)
    for (int ci = 0; ci < Cin; ++ci) {
      const float* g = w + ((size_t)o * Cin + ci) * 9;
      const double sc = scale ? scale[o] : 1.0;
      double t[6][3];
      for (int i = 0; i < n; ++i)
        for (int j = 0; j < 3; ++j)
          t[i][j] = G[i][0] * ((double)g[j] * sc) + G[i][1] * ((double)g[3 + j] * sc) + G[i][2] * ((double)g[6 + j] * sc);
      for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) {
          const double u = t[i][0] * G[j][0] + t[i][1] * G[j][1] + t[i][2] * G[j][2];
          out[((size_t)(n * i + j) * Cout + o) * Cin + ci] = (float)u;
        }
    }
}

void conv_wino64_pack_u(const float* u, float* out) {
  for (int k = 0; k < 36; ++k)
    for (int co = 0; co < 64; ++co)
      for (int ci = 0; ci < 64; ++ci) out[(((size_t)k * 4 + (ci >> 4)) * 64 + co) * 16 + (ci & 15)] = u[((size_t)k * 64 + co) * 64 + ci];
}

// Packed weight rows for the transposed MFMAs: row 32 T + i of the packed matrix is output channel 32 T + sigma(i),
// sigma(i) = 16 ((i >> 2) & 1) + 4 (i >> 3) + (i & 3), so that accumulator register r of lane half h (MFMA row
// (r & 3) + 8 (r >> 2) + 4 h) is channel 32 T + 16 h + r.  `src` is [rows][K] (rows % 32 == 0).
void bottleneck_pack_rows_bf16(const unsigned short* src, int rows, int K, unsigned short* dst) {
  for (int o = 0; o < rows; ++o) {
    const int T = o >> 5, i = o & 31;
    const int sigma = 16 * ((i >> 2) & 1) + 4 * (i >> 3) + (i & 3);
    memcpy(dst + (size_t)o * K, src + (size_t)(32 * T + sigma) * K, (size_t)K * 2);
  }
}

// conv2's weights [256][2304] (rows permuted by bottleneck_pack_rows_bf16, k slice-major) -> the order phase 2's waves of
// bottleneck256_bf16 load them in: [stage 72 of 32 k][channel-tile pair 4][tile of the pair 2][k-step 2][lane 64] pieces of
// 8 k; lane (i, h) of k-step ks holds row 32 (2 cp + c) + i, k = 32 st32 + 16 ks + 8 h .. + 7.
void bottleneck256_pack_w2_frags_bf16(const unsigned short* rows, unsigned short* dst) {
  constexpr int kP = 256;
  for (int st = 0; st < 72; ++st)
    for (int cp = 0; cp < 4; ++cp)
      for (int c = 0; c < 2; ++c)
        for (int ks = 0; ks < 2; ++ks)
          for (int l = 0; l < 64; ++l) {
            const int i = l & 31, h = l >> 5;
            const unsigned short* src = rows + (size_t)(32 * (2 * cp + c) + i) * (9 * kP) + 32 * st + 16 * ks + 8 * h;
            std::copy(src, src + 8, dst + (((((size_t)st * 4 + cp) * 2 + c) * 2 + ks) * 64 + l) * 8);
          }
}

// conv3's weights [1024][256] (rows permuted) -> [64-channel group 16][tile 2][k-step 16][lane 64] pieces of 8 k
void bottleneck256_pack_w3_frags_bf16(const unsigned short* rows, unsigned short* dst) {
  constexpr int kP = 256;
  for (int cq = 0; cq < 16; ++cq)
    for (int c = 0; c < 2; ++c)
      for (int ks = 0; ks < 16; ++ks)
        for (int l = 0; l < 64; ++l) {
          const int i = l & 31, h = l >> 5;
          const unsigned short* src = rows + (size_t)(32 * (2 * cq + c) + i) * kP + 16 * ks + 8 * h;
          std::copy(src, src + 8, dst + ((((size_t)cq * 2 + c) * 16 + ks) * 64 + l) * 8);
        }
}

// ---- whole layouts ----------------------------------------------------------------------------------------------------
namespace {

void pack_rows(const ConvFilter& f, int Cout, int Cin_real, int cin_pad, int k, float* out) {
  conv_pack_weights(f.w, f.scale, Cout, Cin_real, cin_pad, k, k, out);
}
void pack_rows(const ConvFilter& f, int Cout, int Cin_real, int cin_pad, int k, unsigned short* out) {
  conv_pack_weights_bf16(f.w, f.scale, Cout, Cin_real, cin_pad, k, k, out);
}

// [Cout][Kpad(f1) + Kpad(f2)] in T's precision (float, or bf16 bit patterns)
template <typename T>
std::vector<T> side_by_side(const ConvFilter& f1, int Cin_real, int cin_pad, int k, const ConvFilter* f2, int Cin2, int Cout) {
  const int bk = sizeof(T) == 2 ? 64 : kConvBK;
  const int K1 = ceil_div(k * k * cin_pad, bk) * bk, K2 = f2 ? ceil_div(Cin2, bk) * bk : 0;
  std::vector<T> a((size_t)Cout * K1);
  pack_rows(f1, Cout, Cin_real, cin_pad, k, a.data());
  if (!f2) return a;
  std::vector<T> b((size_t)Cout * K2), both((size_t)Cout * (K1 + K2));
  pack_rows(*f2, Cout, Cin2, Cin2, 1, b.data());
  for (int o = 0; o < Cout; ++o) {
    std::copy(&a[(size_t)o * K1], &a[(size_t)o * K1] + K1, &both[(size_t)o * (K1 + K2)]);
    std::copy(&b[(size_t)o * K2], &b[(size_t)o * K2] + K2, &both[(size_t)o * (K1 + K2) + K1]);
  }
  return both;
}

// bf16 bit patterns carried in a float vector, as PlanSink::upload takes every constant
std::vector<float> as_floats(const std::vector<unsigned short>& v) {
  std::vector<float> f((v.size() + 1) / 2);
  memcpy(f.data(), v.data(), v.size() * 2);
  return f;
}

std::vector<unsigned short> permuted_rows(const std::vector<unsigned short>& a, int rows) {
  std::vector<unsigned short> p(a.size());
  bottleneck_pack_rows_bf16(a.data(), rows, (int)(a.size() / rows), p.data());
  return p;
}

std::vector<float> bias_f32(const ConvFilter& f, const ConvFilter* g, int n) {
  std::vector<float> b(n);
  for (int o = 0; o < n; ++o) b[o] = (float)(g ? f.bias[o] + g->bias[o] : f.bias[o]);
  return b;
}

}  // namespace

std::vector<float> conv_pack_side_by_side(const ConvFilter& f1, int Cin_real, int cin_pad, int k, const ConvFilter* f2, int Cin2,
                                          int Cout, int precision) {
  if (precision == 1) return as_floats(side_by_side<unsigned short>(f1, Cin_real, cin_pad, k, f2, Cin2, Cout));
  return side_by_side<float>(f1, Cin_real, cin_pad, k, f2, Cin2, Cout);
}

int bottleneck_pack_bf16(int planes, const ConvFilter& c1, const ConvFilter& c2, const ConvFilter& c3, const ConvFilter* down,
                         BottleneckWeights* out) {
  PR_REQUIRE(planes == 64 || ((planes == 128 || planes == 256) && !down),
             "bottleneck_pack_bf16: %d planes%s has no whole-block kernel", planes, down ? " with a downsample branch" : "");
  PR_REQUIRE(c1.w && c2.w && c3.w && c1.bias && c2.bias && c3.bias && (!down || (down->w && down->bias)), "bottleneck_pack_bf16: null argument");
  const int P = planes, cin = down ? P : 4 * P;
  const std::vector<unsigned short> r1 = permuted_rows(side_by_side<unsigned short>(c1, cin, cin, 1, nullptr, 0, P), P);
  std::vector<unsigned short> r2 = permuted_rows(side_by_side<unsigned short>(c2, P, P, 3, nullptr, 0, P), P);
  std::vector<unsigned short> r3 = permuted_rows(side_by_side<unsigned short>(c3, P, P, 1, down, cin, 4 * P), 4 * P);
  if (P == 256) {      // conv2 and conv3 further into the MFMA fragment orders
    std::vector<unsigned short> g2(r2.size()), g3(r3.size());
    bottleneck256_pack_w2_frags_bf16(r2.data(), g2.data());
    bottleneck256_pack_w3_frags_bf16(r3.data(), g3.data());
    r2.swap(g2);
    r3.swap(g3);
  }
  out->w1 = as_floats(r1);
  out->w2 = as_floats(r2);
  out->w3 = as_floats(r3);
  out->b1 = bias_f32(c1, nullptr, P);
  out->b2 = bias_f32(c2, nullptr, P);
  out->b3 = bias_f32(c3, down, 4 * P);
  return PR_OK;
}

bool expand_res_bf16_fits(int K, int N) { return (K == 128 && N == 512) || (K == 256 && N == 1024); }
bool expand_dual_bf16_fits(int K1, int K2, int N) { return K1 == 128 && K2 == 256 && N == 512; }
bool bottleneck256_bf16_fits(int H, int W) { return H >= 1 && W >= 1 && H * W <= 224; }   // 32 x 7 pixel tiles: kMaxPix of the kernel

// ---- the plan -----------------------------------------------------------------------------------------------------------
namespace {

struct BlobReader {
  const float* p;
  size_t left;
  const float* take(size_t n) {
    if (n > left) return nullptr;
    const float* r = p;
    p += n;
    left -= n;
    return r;
  }
};

size_t hmr_weight_floats_impl() {
  size_t n = 64 * 3 * 49 + 4 * 64;
  int inpl = 64;
  const int planes[4] = {64, 128, 256, 512}, blocks[4] = {3, 4, 6, 3};
  for (int L = 0; L < 4; ++L)
    for (int b = 0; b < blocks[L]; ++b) {
      const int pl = planes[L];
      n += (size_t)pl * inpl + 4 * pl;
      n += (size_t)pl * pl * 9 + 4 * pl;
      n += (size_t)pl * 4 * pl + 4 * pl * 4;
      if (b == 0) n += (size_t)pl * 4 * inpl + 4 * pl * 4;
      inpl = pl * 4;
    }
  n += (size_t)1024 * 2205 + 1024 + (size_t)1024 * 1024 + 1024;
  n += (size_t)144 * 1024 + 144 + 10 * 1024 + 10 + 3 * 1024 + 3 + 144 + 10 + 3;
  return n;
}

struct Ctx {
  HmrPlan* h;
  PlanSink* sink;
  // U of layer1's one-launch Winograd layers, by plan entry: uploaded behind the last convolution's weights (build)
  std::vector<std::pair<size_t, std::vector<float>>> u1_pending;
  int block = 0;      // index of the Bottleneck being planned within its stage (the switch routes layer1 by block)
};

int upload(Ctx& cx, const std::vector<float>& host, float** out) {
  return cx.sink->upload(host.data(), host.size() * sizeof(float), out);
}

int dev_alloc(Ctx& cx, size_t floats, float** out) { return cx.sink->zeros(std::max<size_t>(floats, 4) * sizeof(float), out); }

// One convolution of the blob with its BatchNorm (gamma, beta, mean, var): the raw filter and the BN folded, in
// double, into a per-output-channel scale and bias.
struct FoldedConv {
  const float* w = nullptr;
  std::vector<double> scale, bias;
  ConvFilter filter() const { return {w, scale.data(), bias.data()}; }
};

int read_conv_bn(BlobReader& br, int Cout, int Cin_real, int k, FoldedConv* out) {
  out->w = br.take((size_t)Cout * Cin_real * k * k);
  const float* g = br.take(Cout);
  const float* be = br.take(Cout);
  const float* mu = br.take(Cout);
  const float* var = br.take(Cout);
  PR_REQUIRE(out->w && g && be && mu && var, "hmr: weight blob too short");
  out->scale.resize(Cout);
  out->bias.resize(Cout);
  for (int o = 0; o < Cout; ++o) {
    const double s = (double)g[o] / std::sqrt((double)var[o] + kBnEps);
    out->scale[o] = s;
    out->bias[o] = (double)be[o] - (double)mu[o] * s;
  }
  return PR_OK;
}

// Folded weights of one or two convolutions (two: a conv3 and the downsample branch summed into it) -> device
// rows [Cout][Kpad(f1) + Kpad(f2)] in the handle's precision.
int upload_packed(Ctx& cx, const ConvSpec& spec, const FoldedConv& f1, const FoldedConv* f2, float** out) {
  const ConvFilter g2 = f2 ? f2->filter() : ConvFilter{};
  return upload(cx, conv_pack_side_by_side(f1.filter(), spec.Cin_real, spec.Cin, spec.k, f2 ? &g2 : nullptr, spec.Cin2, spec.Cout, cx.h->precision), out);
}

// A Bottleneck's folded weights in its whole-block kernel's layouts (bottleneck_pack_bf16) -> the block's spec
int upload_block(Ctx& cx, const FoldedConv& f1, const FoldedConv& f2, const FoldedConv& f3, const FoldedConv* fd, ConvSpec* blk) {
  const ConvFilter gd = fd ? fd->filter() : ConvFilter{};
  BottleneckWeights bw;
  PR_TRY(bottleneck_pack_bf16(blk->bneck_planes, f1.filter(), f2.filter(), f3.filter(), fd ? &gd : nullptr, &bw));
  PR_TRY(upload(cx, bw.w1, &blk->w));
  PR_TRY(upload(cx, bw.w2, &blk->w2b));
  PR_TRY(upload(cx, bw.w3, &blk->w3));
  PR_TRY(upload(cx, bw.b1, &blk->bias));
  PR_TRY(upload(cx, bw.b2, &blk->bias2b));
  PR_TRY(upload(cx, bw.b3, &blk->bias3));
  return PR_OK;
}

// conv weight + its BatchNorm -> packed folded weights and bias on device.  `second` (a conv3 whose block has a
// downsample branch, fused form): the branch's conv + BatchNorm follow in the blob and are summed into this conv.
int add_conv(Ctx& cx, BlobReader& br, ConvSpec spec, bool second = false) {
  HmrPlan* const h = cx.h;
  FoldedConv f1, f2;
  std::vector<float> s2d_w;
  if (spec.out_hw) {
    // blob: conv1.weight [64][3][7][7].  8x8 window starting at original pixel (2 ho - 4, 2 wo - 4), i.e. the 7x7
    // kernel with a zero row / column in front; tap (th, tw) of the 4x4 kernel covers original rows 2 th + di:
    //   W2[o][(2 di + dj) * 3 + c][th][tw] = W[o][c][2 th + di - 1][2 tw + dj - 1]   (zero outside 0..6)
    PR_TRY(read_conv_bn(br, spec.Cout, 3, 7, &f1));
    s2d_w.assign((size_t)spec.Cout * 12 * 16, 0.f);
    for (int o = 0; o < spec.Cout; ++o)
      for (int c = 0; c < 3; ++c)
        for (int kh = 0; kh < 7; ++kh)
          for (int kw = 0; kw < 7; ++kw) {
            const int th = (kh + 1) >> 1, di = (kh + 1) & 1, tw = (kw + 1) >> 1, dj = (kw + 1) & 1;
            s2d_w[(((size_t)o * 12 + (2 * di + dj) * 3 + c) * 4 + th) * 4 + tw] = f1.w[(((size_t)o * 3 + c) * 7 + kh) * 7 + kw];
          }
    f1.w = s2d_w.data();
  } else
  PR_TRY(read_conv_bn(br, spec.Cout, spec.Cin_real, spec.k, &f1));
  if (second) PR_TRY(read_conv_bn(br, spec.Cout, spec.Cin2, 1, &f2));
  std::vector<float> bias(spec.Cout);
  for (int o = 0; o < spec.Cout; ++o) bias[o] = (float)(f1.bias[o] + (second ? f2.bias[o] : 0.0));
  PR_TRY(upload_packed(cx, spec, f1, second ? &f2 : nullptr, &spec.w));
  PR_TRY(upload(cx, bias, &spec.bias));
  const float* w = f1.w;
  const std::vector<double>& scale = f1.scale;
  // 3x3 / stride 1 with >= 128 channels (layer2..layer4): the handle's Winograd form as three launches (input transform,
  // grouped GEMMs, output transform).  layer1 (64 channels at 56x56) cannot take that form: V and M would be 115.6 MB each
  // per layer at B = 64, written once and read once, and the passes cost more than the MFMAs they save.  Its conv2 runs as
  // F(4x4,3x3) inside ONE kernel instead (conv_wino64.hip: V and M never leave the CU), on layer2's points when layer2's
  // form is 4 or 5 (stage_form[0], hmr_plan_configure); it is no `wino_m` layer: one launch, no workspace.
  // The form is a property of the handle (pr_hmr_create's conv_form), so one process can hold several.
  const int use_wino = h->stage_form[spec.stage];
  if (spec.stage == 0 && use_wino && (h->wino_layer1 >= 2 || cx.block == 0) && h->precision == 0 && spec.k == 3 && spec.stride == 1 && spec.pad == 1 && spec.Cin == 64 &&
      spec.Cout == 64 && spec.Cin == spec.Cin_real) {
    std::vector<float> u((size_t)36 * 64 * 64), packed(u.size());
    conv_winograd_pack_weights(w, scale.data(), 64, 64, use_wino, u.data());
    conv_wino64_pack_u(u.data(), packed.data());
    cx.u1_pending.emplace_back(h->convs.size(), std::move(packed));
  }
  if (spec.stage > 0 && use_wino && h->precision == 0 && spec.k == 3 && spec.stride == 1 && spec.pad == 1 && spec.Cin >= h->wino_min_c &&
      spec.Cin == spec.Cin_real) {
    const int m = conv_winograd_tile(use_wino), n2 = (m + 2) * (m + 2);
    std::vector<float> u((size_t)n2 * spec.Cout * spec.Cin);
    conv_winograd_pack_weights(w, scale.data(), spec.Cout, spec.Cin, use_wino, u.data());
    PR_TRY(upload(cx, u, &spec.u));
    spec.wino_m = m;
    spec.wino_form = use_wino;
    const size_t tiles = (size_t)((spec.H + m - 1) / m) * ((spec.W + m - 1) / m);
    h->wino_floats_per_frame = std::max(h->wino_floats_per_frame, n2 * tiles * ((size_t)spec.Cin + spec.Cout));
  }
  // bf16: a 128 -> 512 / 256 -> 1024 expansion with residual (conv3 of layer2's and layer3's plain blocks) on the
  // register-resident-weights kernel (the fp32 twin was built and lost: profiles/r03_experiments.txt)
  if (h->precision == 1 && h->expand_regs && spec.k == 1 && spec.stride == 1 && expand_res_bf16_fits(spec.Cin, spec.Cout) &&
      spec.res_buf >= 0 && spec.in2_buf < 0 && !second)
    spec.cfg = kConvCfgExpand;
  // ... and layer2's FIRST conv3 with its downsample branch as the second source of the same kernel
  if (h->precision == 1 && h->expand_regs && spec.k == 1 && spec.stride == 1 && second && spec.in2_buf >= 0 && spec.res_buf < 0 &&
      expand_dual_bf16_fits(spec.Cin, spec.Cin2, spec.Cout))
    spec.cfg = kConvCfgExpand;
  // fp32 1x1 layers with K = 128 or 256 (layer1's conv1, layer2's and layer3's conv3): weights resident in registers.
  // 256 -> 64 at 56x56: 66 us against the tile kernel's 70.5; the wider ones 1 - 3 us ahead or level (profiles/r04_experiments.txt 5)
  if (h->precision == 0 && h->regw && spec.k == 1 && spec.stride == 1 && spec.in2_buf < 0 && !second &&
      (spec.Cin == 128 || spec.Cin == 256) && spec.Cin == spec.Cin_real && spec.Cout % 64 == 0 && spec.cfg < 0)
    spec.cfg = kConvCfgRegW;
  // short-K expansions (layer2's conv3: K = 128; a first block's conv3 + downsample: 64 + 64) as row panels
  {
    const int bk = h->precision == 1 ? 64 : kConvBK;
    if (spec.k == 1 && spec.stride == 1 && spec.Cout > spec.Cin && spec.Cin + spec.Cin2 <= h->panel_max_k &&
        spec.Cin % bk == 0 && spec.Cin2 % bk == 0 && spec.cfg < 0)
      spec.cfg = kConvCfgPanel;
  }
  // The 7x7-map layers with 512 output channels are 49 B / 64 x 8 = 392 tiles at B=64: 1.53 per CU, the launch lasts as
  // long as a CU with two.  Their K (2048 / 4608) is long, so it is dealt to `splitk` workgroups per tile (conv_dma.hip).
  // Decided by the layer's shape only -- never by the batch -- so a frame's bits do not depend on its batch.
  // MEASURED (B=64, POSERISK_SPLITK=2|3|4|6): 3x3/2 layer 158 -> 171 / 177 / 174 / 186 us, the two 1x1 layers 68 -> 89 /
  // 99 / 105 / 133 us: the ticket zeroing launch, the slab round trip and above all one agent-scope release (an L2
  // write-back) per workgroup cost more than the better balance returns.  Off by default (splitk = 1).
  if (h->precision == 0 && h->splitk > 1 && !spec.wino_m && spec.cfg < 0 && spec.in2_buf < 0 && !spec.w3 && spec.Cout == 512 &&
      spec.Ho() == 7 && spec.Cin % kConvBK == 0 && (spec.k == 1 || spec.k == 3))
    spec.splitk = h->splitk;
  h->convs.push_back(spec);
  return PR_OK;
}

// Linear weight [N,K_real] (+bias) -> packed [Npad][Kpad] using columns [col0, col0+K_real) of the
// source row of length src_cols.
int make_fc(Ctx& cx, const float* w, const float* b, int N, int src_cols, int col0, int K_real,
            int Kpad, int Npad, FcSpec* out) {
  std::vector<float> packed((size_t)Npad * Kpad, 0.f), bias(Npad, 0.f);
  for (int n = 0; n < N; ++n) {
    for (int k = 0; k < K_real; ++k) packed[(size_t)n * Kpad + k] = w[(size_t)n * src_cols + col0 + k];
    if (b) bias[n] = b[n];
  }
  out->K = Kpad;
  out->N = Npad;
  PR_TRY(upload(cx, packed, &out->w));
  PR_TRY(upload(cx, bias, &out->bias));
  return PR_OK;
}

int build(Ctx& cx, const float* blob, size_t n_floats) {
  HmrPlan* const h = cx.h;
  BlobReader br{blob, n_floats};
  // stem: conv1 7x7/2 (input padded to 4 channels) -> act[1]; maxpool -> act[2]
  ConvSpec c1{3, h->precision == 1 ? 8 : 4, 64, 7, 2, 3, kImg, kImg, 1, 0, 1, -1};
  if (h->stem_s2d) {
    c1 = ConvSpec{12, h->precision == 1 ? 16 : 12, 64, 4, 1, 2, kImg / 2, kImg / 2, 1, 0, 1, -1};
    c1.out_hw = kImg / 2;
    c1.macs_fixed = (double)(kImg / 2) * (kImg / 2) * 64 * 3 * 49;
  }
  PR_TRY(add_conv(cx, br, c1));
  h->block_last[0] = 0;
  h->block_buf[0] = 2;
  int cur = 2, H = 56, inpl = 64, layer = 1, blk_no = 1;
  const int planes[4] = {64, 128, 256, 512}, blocks[4] = {3, 4, 6, 3};
  for (int L = 0; L < 4; ++L)
    for (int b = 0; b < blocks[L]; ++b) {
      const int pl = planes[L];
      const int stride = (b == 0 && L > 0) ? 2 : 1;
      cx.block = b;
      // pick 4 free buffers among 1..5 other than cur
      int fr[4], nf = 0;
      for (int i = 1; i <= 5 && nf < 4; ++i)
        if (i != cur) fr[nf++] = i;
      const int t1 = fr[0], t2 = fr[1], ds = fr[2], outb = fr[3];
      const int Ho = H / stride;
      ConvSpec a{inpl, inpl, pl, 1, 1, 0, H, H, 1, cur, t1, -1};
      ConvSpec bb{pl, pl, pl, 3, stride, 1, H, H, 1, t1, t2, -1};
      ConvSpec cc{pl, pl, pl * 4, 1, 1, 0, Ho, Ho, 1, t2, outb, b == 0 ? ds : cur};
      a.stage = bb.stage = cc.stage = L;
      if (h->precision == 1 && ((L == 0 && h->fuse_bottleneck && (b > 0 || h->fuse_downsample)) ||
                                (L == 1 && b > 0 && h->fuse_bottleneck2))) {
        // conv1 -> conv2 -> conv3 + identity of this block as ONE launch (bottleneck_bf16.hip): the folded weight
        // matrices in the kernel's layout, one spec; the launch is reported under conv3's index.  The first block's
        // downsample branch rides in conv3's K loop ([t2 | x], as in the dual-source GEMM), its bias summed in double.
        const bool first = b == 0;
        FoldedConv f1, f2, f3, fd;
        PR_TRY(read_conv_bn(br, pl, inpl, 1, &f1));
        PR_TRY(read_conv_bn(br, pl, pl, 3, &f2));
        PR_TRY(read_conv_bn(br, pl * 4, pl, 1, &f3));
        if (first) PR_TRY(read_conv_bn(br, pl * 4, inpl, 1, &fd));
        ConvSpec blk{inpl, inpl, pl * 4, 1, 1, 0, H, H, 1, cur, outb, -1};
        blk.stage = L;
        blk.bneck_planes = pl;
        blk.bneck_first = first;
        PR_TRY(upload_block(cx, f1, f2, f3, first ? &fd : nullptr, &blk));
        layer += first ? 3 : 2;  // conv1, conv2 (and the downsample branch) report no launch of their own
        blk.layer = layer++;
        h->convs.push_back(blk);
        h->block_last[blk_no] = (int)h->convs.size() - 1;
        h->block_buf[blk_no++] = outb;
        cur = outb;
        H = Ho;
        inpl = pl * 4;
        continue;
      }
      const bool alt3 = h->precision == 1 && h->fuse_bottleneck3 && L == 2 && b > 0 && bottleneck256_bf16_fits(H, H);
      if (alt3) {
        // the block's folded weights once more, in bottleneck256_bf16's layouts (the reader is rewound for the three specs below)
        BlobReader again = br;
        FoldedConv f1, f2, f3;
        PR_TRY(read_conv_bn(again, pl, inpl, 1, &f1));
        PR_TRY(read_conv_bn(again, pl, pl, 3, &f2));
        PR_TRY(read_conv_bn(again, pl * 4, pl, 1, &f3));
        HmrPlan::FusedBlock fb;
        fb.first = h->convs.size();
        fb.blk = ConvSpec{inpl, inpl, pl * 4, 1, 1, 0, H, H, 1, cur, outb, -1};
        fb.blk.stage = L;
        fb.blk.bneck_planes = pl;
        PR_TRY(upload_block(cx, f1, f2, f3, nullptr, &fb.blk));
        a.alt3 = (int)h->fused3.size();
        h->fused3.push_back(fb);
      }
      a.layer = layer++;
      bb.layer = layer++;
      PR_TRY(add_conv(cx, br, a));
      PR_TRY(add_conv(cx, br, bb));
      if (b == 0 && h->fuse_downsample) {
        // relu(bn3(conv3(t2)) + bn_d(conv_d(x))) as ONE GEMM over K = [t2's channels | x's channels]: the downsample
        // tensor is never written or read back (execution order: the branch is layer n, conv3 layer n + 1)
        cc.res_buf = -1;
        cc.in2_buf = cur; cc.Cin2 = inpl; cc.H2 = H; cc.stride2 = stride;
        cc.layer2 = layer++;
        cc.layer = layer++;
        PR_TRY(add_conv(cx, br, cc, true));
      } else if (b == 0) {
        // blob order is conv3/bn3 then downsample; execution order is downsample before conv3
        const size_t mark = h->convs.size();
        PR_TRY(add_conv(cx, br, cc));
        ConvSpec dd{inpl, inpl, pl * 4, 1, stride, 0, H, H, 0, cur, ds, -1};
        dd.stage = L;
        PR_TRY(add_conv(cx, br, dd));
        std::swap(h->convs[mark], h->convs[mark + 1]);
        h->convs[mark].layer = layer++;
        h->convs[mark + 1].layer = layer++;
      } else if (L == 0 && h->fuse_conv3) {
        // conv2's 64 output channels are one tile: conv3 + residual + ReLU run on it inside conv2's kernel, and the
        // 64-channel map between them never reaches HBM (conv_fused.hip)
        FoldedConv f3;
        PR_TRY(read_conv_bn(br, cc.Cout, cc.Cin_real, 1, &f3));
        ConvSpec& f = h->convs.back();      // conv2, just added
        std::vector<float> bias3(cc.Cout);
        for (int o = 0; o < cc.Cout; ++o) bias3[o] = (float)f3.bias[o];
        PR_TRY(upload_packed(cx, cc, f3, nullptr, &f.w3));
        PR_TRY(upload(cx, bias3, &f.bias3));
        f.N3 = cc.Cout; f.res3_buf = cc.res_buf; f.out3_buf = cc.out_buf;
        f.layer2 = f.layer;
        f.layer = layer++;
      } else {
        cc.layer = layer++;
        PR_TRY(add_conv(cx, br, cc));
      }
      if (alt3) {
        PR_REQUIRE(h->convs.size() == h->fused3.back().first + 3, "hmr: a plain layer3 block is three launches of the plan");
        h->fused3.back().blk.layer = h->convs.back().layer;   // reported under conv3's index, as the other whole-block kernels
      }
      // every form of the block ends with the entry just added writing outb (conv3, conv3 + downsample, or conv2 carrying conv3)
      h->block_last[blk_no] = (int)h->convs.size() - 1;
      h->block_buf[blk_no++] = outb;
      cur = outb;
      H = Ho;
      inpl = pl * 4;
    }
  h->final_buf = cur;
  for (const auto& pu : cx.u1_pending) PR_TRY(upload(cx, pu.second, &h->convs[pu.first].u1));
  PR_REQUIRE(blk_no == HmrPlan::kBlocks, "hmr: planned %d blocks", blk_no);
  PR_REQUIRE(layer == kNumConv && (int)h->convs.size() ==
                                      kNumConv - (h->fuse_downsample ? 4 : 0) -
                                          (h->precision == 1 && h->fuse_bottleneck ? (h->fuse_downsample ? 6 : 4) : h->fuse_conv3 ? 2 : 0) -
                                          (h->precision == 1 && h->fuse_bottleneck2 ? 6 : 0),
             "hmr: planned %d convolutions in %zu launches, expected %d", layer, h->convs.size(), kNumConv);

  const float* fc1w = br.take((size_t)1024 * 2205);
  const float* fc1b = br.take(1024);
  const float* fc2w = br.take((size_t)1024 * 1024);
  const float* fc2b = br.take(1024);
  const float* dpw = br.take((size_t)144 * 1024);
  const float* dpb = br.take(144);
  const float* dsw = br.take((size_t)10 * 1024);
  const float* dsb = br.take(10);
  const float* dcw = br.take((size_t)3 * 1024);
  const float* dcb = br.take(3);
  const float* ip = br.take(144);
  const float* is = br.take(10);
  const float* ic = br.take(3);
  PR_REQUIRE(fc1w && fc1b && fc2w && fc2b && dpw && dpb && dsw && dsb && dcw && dcb && ip && is && ic,
             "hmr: weight blob too short");
  PR_REQUIRE(br.left == 0, "hmr: weight blob has %zu trailing floats", br.left);
  PR_TRY(make_fc(cx, fc1w, fc1b, 1024, 2205, 0, 2048, 2048, 1024, &h->fc1x));
  PR_TRY(make_fc(cx, fc1w, nullptr, 1024, 2205, 2048, 157, kStateStride, 1024, &h->fc1s));
  PR_TRY(make_fc(cx, fc2w, fc2b, 1024, 1024, 0, 1024, 1024, 1024, &h->fc2));
  {
    std::vector<float> decw((size_t)157 * 1024), decb(157);
    std::copy(dpw, dpw + (size_t)144 * 1024, decw.begin());
    std::copy(dsw, dsw + (size_t)10 * 1024, decw.begin() + (size_t)144 * 1024);
    std::copy(dcw, dcw + (size_t)3 * 1024, decw.begin() + (size_t)154 * 1024);
    std::copy(dpb, dpb + 144, decb.begin());
    std::copy(dsb, dsb + 10, decb.begin() + 144);
    std::copy(dcb, dcb + 3, decb.begin() + 154);
    PR_TRY(make_fc(cx, decw.data(), decb.data(), 157, 1024, 0, 1024, 1024, kStateStride, &h->dec));
  }
  {
    std::vector<float> init(160, 0.f);
    std::copy(ip, ip + 144, init.begin());
    std::copy(is, is + 10, init.begin() + 144);
    std::copy(ic, ic + 3, init.begin() + 154);
    PR_TRY(upload(cx, init, &h->init157));
  }

  // workspaces
  const size_t B = (size_t)h->max_batch;
  PR_TRY(dev_alloc(cx, B * 2048, &h->xf));
  PR_TRY(dev_alloc(cx, B * 1024, &h->h_static));
  PR_TRY(dev_alloc(cx, B * 1024, &h->h1));
  PR_TRY(dev_alloc(cx, B * 1024, &h->h2));
  PR_TRY(dev_alloc(cx, B * kStateStride, &h->state));
  return PR_OK;
}

}  // namespace

size_t hmr_weight_floats() { return hmr_weight_floats_impl(); }

bool hmr_conv_form_valid(int conv_form) {
  auto form_ok = [](int f) { return f == 0 || f == 2 || f == 4 || f == 5; };
  return conv_form == PR_CONV_FORM_DEFAULT || form_ok(conv_form) ||
         (conv_form >= 100 && conv_form <= 555 && form_ok(conv_form / 100) && form_ok(conv_form / 10 % 10) && form_ok(conv_form % 10));
}

void hmr_plan_configure(HmrPlan* h, int precision, int conv_form, int max_batch) {
  auto form_ok = [](int f) { return f == 0 || f == 2 || f == 4 || f == 5; };
  h->max_batch = max_batch;
  h->precision = precision;
  if (conv_form == PR_CONV_FORM_DEFAULT) {
    // POSERISK_WINOGRAD in the environment only moves the default (A/B runs of unmodified callers); an explicit
    // conv_form always wins
    conv_form = PR_CONV_FORM_BUILTIN_DEFAULT;
    if (const char* e = getenv("POSERISK_WINOGRAD")) {
      const int v = atoi(e);
      conv_form = (v == 2 || v == 4 || v == 5 || (v >= 100 && v <= 555)) ? v : 0;
    }
  }
  h->conv_form = conv_form;
  for (int st = 1; st < 4; ++st) {
    const int f = conv_form >= 100 ? (st == 1 ? conv_form / 100 : st == 2 ? conv_form / 10 % 10 : conv_form % 10) : conv_form;
    h->stage_form[st] = form_ok(f) ? f : 0;
  }
  // A/B switches: every one is read here, once per handle, into a handle field (nothing is latched per process)
  if (const char* e = getenv("POSERISK_FC_TILES")) h->fc_tiles = atoi(e);
  if (const char* e = getenv("POSERISK_FC_SHAPE")) h->fc_shape = atoi(e);                      // A/B timing only (same bits)
  if (const char* e = getenv("POSERISK_WINOGRAD_MIN_C")) h->wino_min_c = atoi(e);
  if (const char* e = getenv("POSERISK_FUSE_DOWNSAMPLE")) h->fuse_downsample = atoi(e) != 0;   // A/B timing only
  if (const char* e = getenv("POSERISK_FUSE_CONV3")) h->fuse_conv3 = atoi(e) != 0;             // A/B timing only
  if (const char* e = getenv("POSERISK_STEM_S2D")) h->stem_s2d = atoi(e) != 0;                 // A/B timing only
  if (const char* e = getenv("POSERISK_FUSE_BOTTLENECK")) h->fuse_bottleneck = atoi(e) != 0;   // A/B timing only
  if (const char* e = getenv("POSERISK_FUSE_BOTTLENECK2")) h->fuse_bottleneck2 = atoi(e) != 0; // A/B timing only
  if (const char* e = getenv("POSERISK_FUSE_STEM")) h->fuse_stem = atoi(e) != 0;               // A/B timing only
  if (const char* e = getenv("POSERISK_EXPAND_REGS")) h->expand_regs = atoi(e) != 0;           // A/B timing only
  if (const char* e = getenv("POSERISK_FUSE_BOTTLENECK3")) h->fuse_bottleneck3 = atoi(e) != 0; // A/B timing only
  if (const char* e = getenv("POSERISK_B128_LEAD")) h->b128_lead = atoi(e);                    // A/B timing only
  if (const char* e = getenv("POSERISK_BALANCED")) h->balanced = atoi(e) != 0;                 // A/B timing only
  if (precision == 1) h->panel_max_k = 0;   // bf16: off until measured (POSERISK_PANEL_MAX_K)
  if (const char* e = getenv("POSERISK_PANEL_MAX_K")) h->panel_max_k = atoi(e);                // A/B timing only (0 = off)
  if (const char* e = getenv("POSERISK_REGW")) h->regw = atoi(e) != 0;                         // A/B timing only
  if (const char* e = getenv("POSERISK_SPLITK")) h->splitk = std::max(1, std::min(atoi(e), 8));    // A/B timing only (1 = off)
  if (const char* e = getenv("POSERISK_WINO_LAYER1")) h->wino_layer1 = std::max(0, std::min(atoi(e), 2));   // 0 | 1 | 2 (changes layer1's rounding)
  // layer1 follows layer2's form where that is an F(4x4,3x3) one (the one-launch kernel has no F(2x2) form)
  h->stage_form[0] = precision == 0 && h->wino_layer1 && (h->stage_form[1] == 4 || h->stage_form[1] == 5) ? h->stage_form[1] : 0;
}

int hmr_plan_build(HmrPlan* plan, const float* blob, size_t n_floats, PlanSink& sink) {
  PR_REQUIRE(plan && blob, "hmr plan: null argument");
  PR_REQUIRE(n_floats == hmr_weight_floats(), "pr_hmr_create: blob has %zu floats, expected %zu", n_floats, hmr_weight_floats());
  PR_REQUIRE(plan->max_batch > 0 && plan->max_batch <= 4096, "pr_hmr_create: max_batch %d out of range", plan->max_batch);
  Ctx cx{plan, &sink};
  return build(cx, blob, n_floats);
}

HmrChunkSizes hmr_chunk_sizes(const HmrPlan& plan, int chunk_cap) {
  HmrChunkSizes z{};
  const size_t cb = (size_t)chunk_cap;
  const size_t fmap = (size_t)112 * 112 * 64;  // == 56*56*256, the largest feature map per frame
  // element counts; bf16 buffers hold the same number of elements in half the bytes (input: 8 channels)
  z.act0_floats = cb * kImg * kImg * 4;
  z.act_floats = plan.precision == 1 ? (cb * fmap + 1) / 2 : cb * fmap;
  z.wino_floats = cb * plan.wino_floats_per_frame;
  for (const ConvSpec& cs : plan.convs)
    if (cs.splitk > 1) {
      const size_t tiles = (size_t)ceil_div((int)(cb * cs.Ho() * cs.Wo()), 64) * (cs.Cout / 64);
      z.slab_floats = std::max(z.slab_floats, tiles * cs.splitk * 4096);
      z.tickets = std::max(z.tickets, tiles);
    }
  return z;
}

int hmr_split_batch(int B, int chunk_cap, int n_chunks, bool serial, int* sizes, int max_sizes, bool* concurrent) {
  int nch = serial ? 1 : std::min(n_chunks, B);
  if (nch > 1 && ceil_div(B, nch) > chunk_cap) nch = 1;   // larger than the concurrent buffers: serial passes
  int n = 0;
  if (nch <= 1) {
    for (int b0 = 0; b0 < B && n < max_sizes; b0 += chunk_cap) sizes[n++] = std::min(chunk_cap, B - b0);
  } else {
    for (int c = 0; c < nch && n < max_sizes; ++c) sizes[n++] = (int)((long)(c + 1) * B / nch) - (int)((long)c * B / nch);
  }
  if (concurrent) *concurrent = nch > 1;
  return n;
}

// ---- which kernel -------------------------------------------------------------------------------------------------------
namespace {

// The first-generation kernel (register-staged operands, padded LDS rows; configs 0-5) was retired in round 3: production ran
// on the LDS-DMA kernels since round 1 and the parity tests compare every configuration with torch, not with it.  The 256x256
// bf16 tile (config 18, round 6) was retired too: 25-60 % slower on the shapes it was built for (profiles/r06_tile256_bf16.txt)
// and never picked.
constexpr int kNumCfg = 19;
const ConvTileCfg kCfgs[kNumCfg] = {
    {128, 128, 256, "reg_128x128x32_w2x2", 2, false},
    {128, 64, 256, "reg_128x64x32_w2x2", 2, false},
    {64, 64, 256, "reg_64x64x32_w2x2", 4, false},
    {256, 128, 512, "reg_256x128x32_w4x2", 1, false},
    {64, 128, 256, "reg_64x128x32_w2x2", 2, false},
    {256, 64, 512, "reg_256x64x32_w4x2", 1, false},
    {128, 128, 256, "dma_128x128x32_w2x2", 2},
    {128, 64, 256, "dma_128x64x32_w2x2", 3},
    {64, 64, 256, "dma_64x64x32_w2x2", 5},
    {256, 128, 512, "dma_256x128x32_w4x2", 1},
    {64, 128, 256, "dma_64x128x32_w2x2", 3},
    {256, 64, 512, "dma_256x64x32_w4x2", 2},
    {128, 128, 512, "dma_128x128x32_w4x2", 2},   // 8 waves per 128x128 tile (32x64 per wave)
    {128, 64, 512, "dma_128x64x32_w4x2", 3},     // 8 waves per 128x64 tile (32x32 per wave)
    {64, 64, 128, "dma_64x64x32_w2x1", 5},       // 2 waves per 64x64 tile (32x64 per wave)
    {128, 64, 128, "dma_128x64x32_w2x1", 3},     // 2 waves per 128x64 tile (64x64 per wave)
    {64, 128, 128, "dma_64x128x32_w1x2", 3},     // 2 waves per 64x128 tile (64x64 per wave)
    {64, 256, 256, "dma_64x256x32_w2x2", 2},     // whole 256-channel rows per tile (32x128 per wave): short-K conv3
    {256, 256, 512, "dma_256x256x64_w4x2_bf16", 1, false},   // bf16 only, two-pass epilogue; retired
};

}  // namespace

int conv_num_tile_cfgs() { return kNumCfg; }
const ConvTileCfg* conv_tile_cfg(int cfg) { return cfg >= 0 && cfg < kNumCfg ? &kCfgs[cfg] : nullptr; }

int conv_pick_tile_cfg(const ConvShape& p, const ConvTuning& tune) {
  // Experiment hook (ConvTuning::force_cfg): one tile configuration wherever it fits.
  const int forced = tune.force_cfg;
  // (fp32 dual-source and split-K launches exist on the 64x64 tile only: they keep it)
  const bool fixed_tile = p.precision == 0 && (p.second || p.splitk > 1);
  // (a retired index is handed on like a live one: conv_launch refuses it by name, in both precisions)
  if (forced >= 0 && forced < kNumCfg && !fixed_tile && p.Cout % kCfgs[forced].BN == 0 && p.M >= kCfgs[forced].BM) return forced;
  if (p.precision == 1) {
    // bf16: the MFMA is 16x faster, so the kernel lives on L2->LDS bandwidth and wants big tiles.  Per-layer times inside
    // the B=256 pipeline, every tile configuration in turn (gpurun_out/r02_layers256_bf16_cfg*.txt; round 1's isolated
    // sweep without residuals had put the 256x64 tile first): the 8-wave 128x128 tile (32x64 per wave) is the fastest on
    // every layer with >= 128 output channels (4.18 ms of conv per step against 4.49 with 256x64) except layer2's short-K
    // expansions with residual, where 128x64 wins (125 vs 140 us); 64-channel 1x1 layers take 128x64, the stem and
    // layer1's 3x3 keep 256x64 (all tiles within 1 %).  The tile index goes by the rows of the launch:
    if (p.Cout % 128 == 0 && p.M >= 128) return (p.KH == 1 && !p.second && p.residual && p.Cin <= 128) ? 13 : 12;
    if (p.M >= 256) return p.KH == 1 ? 13 : 11;
    return 8;
  }
  // fp32: the 4-wave 64x64 LDS-DMA tile (5 workgroups per CU, quarter tiles for the remainder).  Sweeps of all 23
  // ResNet-50 shapes at B=64 and B=256 (profiles/r01_conv_tile_sweep_b64.txt, ..._b256_fp32.txt): it is the fastest or
  // within a few percent of the fastest configuration on every shape; an earlier cost model that weighed tile
  // efficiency against quantisation picked larger tiles at B=256 and lost 10 % of the conv time there.
  return 8;
}

bool conv_bal_bf16_fits(const ConvShape& p) {
  if (p.precision != 1 || p.groups != 1 || p.conv3 || p.residual || p.KH != p.KW) return false;
  if (p.Cout % 128 || p.Cin % 64) return false;
  if (p.second && (p.KH != 1 || p.Cin2 % 64 || p.stride2 <= 0)) return false;   // a second source: 1x1 only
  if (p.KH == 1) return p.pad == 0;
  return p.KH == 3;
}

// Where it pays.  MEASURED inside the encoder at B = 256, same box, per layer (profiles/r03_conv_bal.txt): the layers with
// 256-channel blocks and runs of >= 6 pixel tiles gain 7-13 % (layer3's conv1 / conv2, the first conv1 of layer3 and
// layer4); with 3 tiles per run the weights a workgroup streams per chunk outweigh its pixels (layer4: 0.8x the tile
// kernel stand-alone).  Of the layers with 128 output channels only layer2's first conv1 gains (4 %); the others read
// a tensor the expansion kernel has just written and lose 2-12 % against the tile kernel's order of tiles.
// The outputs are the tile kernel's bit for bit, so the choice may depend on the batch.
bool conv_bal_bf16_pays(const ConvShape& p, int cus) {
  if (!conv_bal_bf16_fits(p)) return false;
  const int nb = p.Cout / (p.Cout % 256 == 0 ? 256 : 128);
  const int runs = std::max(cus / (8 * nb), 1) * 8;
  if (ceil_div(p.M, 32) < 6 * runs) return false;
  return p.Cout % 256 == 0 || (p.KH == 1 && p.Cin <= 256);
}

bool conv_regw_f32_fits(const ConvShape& p) {
  return p.precision == 0 && p.KH == 1 && p.KW == 1 && p.stride == 1 && p.pad == 0 && !p.second && !p.conv3 && p.groups >= 1 &&
         (p.groups == 1 || (!p.bias && !p.residual && !p.relu)) && p.splitk == 1 && (p.Cin == 128 || p.Cin == 256) &&
         p.Cout % 64 == 0 && p.M > 0;
}

HmrRoute hmr_route(const HmrPlan& plan, const ConvTuning& tune, size_t ci, int b) {
  const ConvSpec& c = plan.convs[ci];
  HmrRoute r{HmrKernel::Tile, -1, &c, 1, c.layer};
  if (c.alt3 >= 0 && hmr_fused3_pays(b, plan.cus)) {      // the block's other two entries: done by the whole-block kernel
    const ConvSpec* blk = &plan.fused3[c.alt3].blk;
    r = HmrRoute{HmrKernel::Bottleneck, -1, blk, 3, blk->layer};
  } else if (ci == 0 && plan.stem_s2d && plan.fuse_stem) r.kernel = HmrKernel::StemPool;      // the stem and its max-pool as one launch
  else if (c.bneck_planes) r.kernel = HmrKernel::Bottleneck;
  else if (c.u1) r.kernel = HmrKernel::Wino64;        // layer1's conv2 (+ conv3) as one-launch F(4x4,3x3)
  else if (c.u) r.kernel = HmrKernel::Winograd;       // three launches (transform, grouped GEMMs, transform), timed as one conv
  else {
    const ConvShape s = c.shape(plan.precision, b);
    r.cfg = c.cfg >= 0 ? c.cfg : conv_pick_tile_cfg(s, tune);
    if (plan.precision == 1 && plan.balanced && c.cfg < 0 && conv_bal_bf16_pays(s, plan.cus)) r.cfg = kConvCfgBalanced;
    r.kernel = s.conv3 ? HmrKernel::Fused3 : r.cfg == kConvCfgPanel ? HmrKernel::Panel : r.cfg == kConvCfgRegW ? HmrKernel::RegW
               : r.cfg == kConvCfgExpand ? HmrKernel::Expand : r.cfg == kConvCfgBalanced ? HmrKernel::Balanced : HmrKernel::Tile;
  }
  return r;
}

void hmr_plan_counts(const HmrPlan& plan, int B, int chunk_cap, int n_chunks, bool serial, int* conv_launches, int* winograd_layers) {
  // as encode_chunks walks the plan, once per sub-batch pr_hmr_forward really runs: the last serial pass is shorter and
  // concurrent shares are B / n frames each, and whether a whole-block kernel pays is decided per sub-batch (no count
  // depends on the tile choice: the default tuning serves)
  std::vector<int> sizes((size_t)std::max(n_chunks, ceil_div(std::max(B, 1), std::max(chunk_cap, 1))) + 1);
  const int n = hmr_split_batch(B, chunk_cap, n_chunks, serial, sizes.data(), (int)sizes.size(), nullptr);
  int launches = 0, wino = 0;
  for (int i = 0; i < n; ++i)
    for (size_t ci = 0; ci < plan.convs.size();) {
      const HmrRoute r = hmr_route(plan, ConvTuning{}, ci, sizes[i]);
      ++launches;
      wino += r.kernel == HmrKernel::Winograd;
      ci += r.span;
    }
  if (conv_launches) *conv_launches = launches;
  if (winograd_layers) *winograd_layers = wino;
}

}  // namespace pr
