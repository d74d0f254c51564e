// The device-free half of pr_hmr_create: everything between the caller's weight blob and what the kernels launch.
// (SPIN models/hmr.py as lib/core/base.py:81-84 builds and loads it: hmr(cfg.SPIN.SMPL_MEAN_PARAMS) + load_state_dict.)
//
//   * the canonical blob's layout and size (include/poserisk_hip.h);
//   * eval-mode BatchNorm folded into every convolution, in double;
//   * weight packing for every kernel family: [Cout][K] fp32 and bf16 rows, the space-to-depth stem, the Winograd-domain
//     weights U = G g G^T, the row permutation of the transposed-MFMA kernels, the fragment orders of bottleneck256_bf16,
//     and over them the whole layouts (two matrices side by side, a Bottleneck for its whole-block kernel), defined once for
//     the plan and for the stand-alone test entries of capi.hip;
//   * the 53-convolution execution plan: which launch carries which layer, buffer rotation, fusions;
//   * kernel routing: the kernels' shape predicates (over ConvShape) and hmr_route, the ONE place that decides which kernel
//     carries a plan entry at b frames -- hmr.hip's encode_chunks, hmr_plan_counts and the walkers under tests/native follow it;
//   * workspace sizes per sub-batch, and what a forward of B frames launches.
//
// Nothing here includes a HIP header: device memory is reached through PlanSink.  The library's sink allocates and copies
// with HIP (hmr.hip); tests/native/host_plan_check.cc builds this file with g++ -fsanitize=address,undefined and a sink
// over host memory (SURVEY.md section 5 asks for a sanitizer build of the host C++; this code otherwise only ever runs
// behind pr_hmr_create, which needs a GPU).
#pragma once
#include <algorithm>
#include <cstdlib>
#include <vector>

#include "host_common.h"

namespace pr {

constexpr int kConvBK = 32;        // floats of K per LDS stage of the fp32 kernels: packed fp32 rows are padded to it
constexpr int kStateStride = 192;  // regressor state row: pose6d(144) | betas(10) | cam(3) | zero pad
constexpr int kImg = 224;
constexpr double kBnEps = 1e-5;
constexpr int kNumConv = 53;
constexpr int kHmrMaxChunks = 8;

// conv_launch routes (conv_igemm.h lists the kernels behind them)
constexpr int kConvCfgPanel = 100;
constexpr int kConvCfgExpand = 300;
constexpr int kConvCfgBalanced = 301;
constexpr int kConvCfgRegW = 400;

// ---- weight packing (pure host) --------------------------------------------------------------------------------
// PyTorch OIHW float weights (+ optional per-output-channel scale, applied in double) -> packed [Cout][Kpad], k = (kh KW +
// kw) cin_pad + ci, zero padded to a multiple of kConvBK.
void conv_pack_weights(const float* w_oihw, const double* scale, int Cout, int Cin_real, int cin_pad, int KH, int KW,
                       float* out_packed);
// bf16 twin: K padded to a multiple of 64, k order by conv_k_index_bf16.
void conv_pack_weights_bf16(const float* w_oihw, const double* scale, int Cout, int Cin_real, int cin_pad, int KH, int KW,
                            unsigned short* out_packed);
int conv_kpad_bf16(int K);
// Position of (tap, ci) in a packed bf16 weight row.  Kernels with more than one tap and Cin % 64 == 0 run their K loop
// SLICE-major: k = (ci / 64) * taps * 64 + tap * 64 + ci % 64 -- all taps of a 64-channel slice before the next slice, so
// a kernel can keep a slice's pixel block in LDS across the taps (bottleneck_bf16.hip does for its one slice; the
// multi-slice form was built and measured in round 3, profiles/r03_experiments.txt); one slice (Cin = 64) is the plain
// tap-major order.  Otherwise (the stem) k = tap * Cin + ci.
inline int conv_k_index_bf16(int tap, int ci, int taps, int cin_pad) {
  if (taps > 1 && cin_pad % 64 == 0) return (ci >> 6) * taps * 64 + tap * 64 + (ci & 63);
  return tap * cin_pad + ci;
}
unsigned short f32_to_bf16_host(float f);

// Winograd F(m x m, 3x3): `form` 2 = F(2x2,3x3), 4 = F(4x4,3x3) on Lavin & Gray's points 0, +-1, +-2, 5 = F(4x4,3x3) on
// 0, +-kWa, +-kWb (half the fp32 error of form 4 at the same cost; conv_winograd.hip).  U = G g G^T in double with the
// BatchNorm scale folded first, one rounding to fp32, layout [(m+2)^2][Cout][Cin].
constexpr float kWa = 11.f / 16.f, kWb = 3.f / 2.f;
inline int conv_winograd_tile(int form) { return form == 2 ? 2 : 4; }
void conv_winograd_pack_weights(const float* w_oihw, const double* scale, int Cout, int Cin, int form, float* out_u);
// The one-launch F(4x4,3x3) kernel of the 64 -> 64 channel layers (conv_wino64.hip) walks the input channels in four slices
// of 16: U [36][64 co][64 ci] as conv_winograd_pack_weights leaves it -> [36][4 slices][64 co][16 ci], a wave's fragment of a
// plane and slice one contiguous KB.  kWino64Tiles: tiles per workgroup = the B columns of its MFMA.
constexpr int kWino64Tiles = 16;
void conv_wino64_pack_u(const float* u, float* out);

// Packed weight rows for the transposed MFMAs of the whole-Bottleneck kernels: row 32 T + i of the packed matrix is output
// channel 32 T + sigma(i), sigma(i) = 16 ((i >> 2) & 1) + 4 (i >> 3) + (i & 3).  `src` is [rows][K] (rows % 32 == 0).
void bottleneck_pack_rows_bf16(const unsigned short* src, int rows, int K, unsigned short* dst);
// bottleneck256_bf16.hip's fragment orders of conv2's [256][2304] and conv3's [1024][256] permuted rows
void bottleneck256_pack_w2_frags_bf16(const unsigned short* rows, unsigned short* dst);
void bottleneck256_pack_w3_frags_bf16(const unsigned short* rows, unsigned short* dst);

// ---- whole layouts: the one definition of each, for the plan (build) and the stand-alone test entries (capi.hip) alike ----
// One convolution as the packers below take it: the OIHW filter, the per-output-channel scale its BatchNorm folds to
// (applied in double; null = the filter is already folded) and its bias (null = none).
struct ConvFilter {
  const float* w = nullptr;
  const double* scale = nullptr;
  const double* bias = nullptr;
};
// Rows [Cout][Kpad(k k cin_pad) + Kpad(Cin2)] of `f1` (k x k) and, side by side with it, of the 1x1 `f2` (null = none; a
// conv3 with the downsample branch summed into it), Kpad by the precision.  precision 1: bf16 bit patterns, two to a float.
std::vector<float> conv_pack_side_by_side(const ConvFilter& f1, int Cin_real, int cin_pad, int k, const ConvFilter* f2, int Cin2,
                                          int Cout, int precision);
// A Bottleneck's weights as the whole-block kernel of its `planes` reads them (64: bottleneck_bf16.hip, 128: bottleneck128_bf16.hip,
// 256: bottleneck256_bf16.hip): w1 / w2 / w3 bf16 (two to a float) with the rows permuted by bottleneck_pack_rows_bf16, 256
// planes further into the fragment orders; biases fp32 in channel order.  `down` (64 planes only: the stage's first block,
// 64-channel input): the downsample branch rides in conv3's K loop, w3 = [conv3 | down] side by side, b3 their sum in double.
struct BottleneckWeights {
  std::vector<float> w1, w2, w3, b1, b2, b3;
};
int bottleneck_pack_bf16(int planes, const ConvFilter& c1, const ConvFilter& c2, const ConvFilter& c3, const ConvFilter* down,
                         BottleneckWeights* out);

// shape predicates of the kernels the plan routes to (pure; the kernels' own launchers re-check them)
bool expand_res_bf16_fits(int K, int N);
bool expand_dual_bf16_fits(int K1, int K2, int N);
bool bottleneck256_bf16_fits(int H, int W);

// What a kernel choice may read of a convolution launch: integers and whether a tensor is there.  Two producers:
// ConvProblem::shape() (conv_igemm.h) and ConvSpec::shape(precision, b), a plan entry at b frames as hmr.hip's conv_problem fills it in.
struct ConvShape {
  int precision = 0, groups = 1, M = 0, Cin = 0, Cout = 0, KH = 1, KW = 1, stride = 1, pad = 0, Cin2 = 0, stride2 = 1, splitk = 1;
  bool second = false, residual = false, conv3 = false, bias = false, relu = false;   // x2 / res / w3 / bias given; ReLU
};

// ---- the plan -------------------------------------------------------------------------------------------------
struct ConvSpec {
  int Cin_real, Cin, Cout, k, stride, pad, H, W;  // input H,W
  int relu;
  int in_buf, out_buf, res_buf;  // activation buffer ids (res_buf < 0: none)
  float* w = nullptr;            // device, packed
  float* bias = nullptr;         // device
  float* u = nullptr;            // device, Winograd-domain weights [(m+2)^2][Cout][Cin] (3x3 stride-1 layers of layer2..4)
  int wino_m = 0;                // Winograd output tile (2 or 4), 0 = direct form
  int wino_form = 0;             // ... and the form it belongs to (2, 4, or 5 = F(4x4) on the points 0, +-11/16, +-3/2)
  // A 64 -> 64 channel 3x3 / stride-1 layer (layer1's conv2) as F(4x4,3x3) inside ONE kernel (conv_wino64.hip), with or
  // without the conv3 of `w3` behind it: U in conv_wino64_pack_u's layout, built on the form of HmrPlan::stage_form[0] (4 or
  // 5).  Not a `wino_m` layer: one launch, no V / M workspace.
  float* u1 = nullptr;
  int cfg = -1;
  int layer = 0;                 // index among the 53 convolutions of the network (execution order), for the profile
  int stage = 0;                 // ResNet stage 0..3 (layer1..layer4); the stem counts as stage 0
  // A first Bottleneck's downsample branch summed into its conv3 (one K loop over [conv2 output | block input],
  // conv_igemm.h ConvProblem::x2): the block input's buffer, channels, size and the branch's stride.
  int in2_buf = -1, Cin2 = 0, H2 = 0, stride2 = 1, layer2 = -1;
  // The block's conv3 applied inside this (3x3, 64-channel) convolution's kernel (conv_fused.hip): packed weights and
  // bias, output channels, residual and output buffers.
  float* w3 = nullptr;
  float* bias3 = nullptr;
  int N3 = 0, res3_buf = -1, out3_buf = -1;
  // The stem after space-to-depth: a 4x4 / stride-1 convolution over 12 channels of the 112x112 map whose window starts
  // two pixels up-left (pad 2) and ends one pixel down-right, so the output size is given, not derived; its algorithmic
  // work stays the 7x7 convolution's.
  int out_hw = 0;
  double macs_fixed = 0;
  int splitk = 1;                // K-steps of every tile dealt to this many workgroups (a property of the layer)
  // A whole Bottleneck in one kernel (bottleneck_bf16.hip; bf16 layer1 blocks without a downsample branch): this spec is
  // the block (in_buf -> out_buf, Cin = Cout = 4 * planes); w / bias are conv1's, w2b / bias2b conv2's, w3 / bias3 conv3's
  // (rows permuted by bottleneck_pack_rows_bf16).
  int bneck_planes = 0;
  bool bneck_first = false;      // the stage's first block: 64-channel input, downsample branch in conv3's K loop
  float* w2b = nullptr;
  float* bias2b = nullptr;
  int alt3 = -1;                 // the first of a plain layer3 block's three entries: index of its alternate in HmrPlan::fused3
  ConvShape shape(int precision, int b) const {
    ConvShape s;
    s.precision = precision; s.M = b * Ho() * Wo(); s.Cin = Cin; s.Cout = Cout; s.KH = s.KW = k; s.stride = stride; s.pad = pad; s.splitk = splitk;
    s.second = in2_buf >= 0; s.residual = res_buf >= 0; s.conv3 = w3 && out3_buf >= 0; s.bias = bias != nullptr; s.relu = relu != 0;
    if (s.second) { s.Cin2 = Cin2; s.stride2 = stride2; }
    return s;
  }
  int Ho() const { return out_hw ? out_hw : (H + 2 * pad - k) / stride + 1; }
  int Wo() const { return out_hw ? out_hw : (W + 2 * pad - k) / stride + 1; }
  double macs_per_frame() const {
    if (bneck_planes)      // 1x1 (4P -> P, first block P -> P) + 3x3 (P -> P) + 1x1 (P -> 4P) (+ the first block's P -> 4P branch)
      return (double)H * W * bneck_planes * bneck_planes * (bneck_first ? 18.0 : 17.0);
    return macs_fixed > 0 ? macs_fixed : (double)Ho() * Wo() * (Cout * (Cin_real * k * k + Cin2) + (double)N3 * Cout);
  }
  // Multiply-adds the matrix pipes really execute per frame: the packed K (zero padding included) for direct layers,
  // (m+2)^2 products per m x m output tile for a Winograd layer.
  double mfma_macs_per_frame(int k_step) const {
    if (bneck_planes) return macs_per_frame();
    if (u1) {      // 36 products per 4x4 tile, the idle B columns of a unit's last MFMA included, + conv3 as it stands
      const int cols = ((W + 3) / 4 + kWino64Tiles - 1) / kWino64Tiles * kWino64Tiles;      // rounded up in integers
      return (double)((H + 3) / 4) * cols * 36 * Cin * Cout + (double)Ho() * Wo() * N3 * Cout;
    }
    if (wino_m) {
      const double tiles = (double)((H + wino_m - 1) / wino_m) * ((W + wino_m - 1) / wino_m);
      return tiles * (wino_m + 2) * (wino_m + 2) * Cin * Cout;
    }
    const int kp = (k * k * Cin + k_step - 1) / k_step * k_step;
    return (double)Ho() * Wo() * (Cout * (double)(kp + Cin2) + (double)N3 * Cout);
  }
};

struct FcSpec {  // y[B,N] = x[B,K] * W^T (+bias) (+res)
  int K = 0, N = 0;
  float* w = nullptr;
  float* bias = nullptr;
};

// Where the plan's constants go.  upload: a device copy of `bytes` host bytes; zeros: a zero-filled device buffer.
struct PlanSink {
  virtual int upload(const void* host, size_t bytes, float** out) = 0;
  virtual int zeros(size_t bytes, float** out) = 0;
  virtual ~PlanSink() = default;
};

// Settings + plan of one handle.  pr_hmr (hmr.hip) derives from it and adds the device state.
struct HmrPlan {
  int max_batch = 0;
  int precision = 0;  // 0 = fp32 encoder, 1 = bf16 encoder (fp32 accumulate); the regressor is always fp32
  int conv_form = PR_CONV_FORM_BUILTIN_DEFAULT;  // fp32 encoder: 0 = every conv direct, 2 / 4 / 5 = a Winograd form, or a digit per stage
  int stage_form[4] = {0, 5, 5, 5};  // the form per ResNet stage (layer1: 0 = direct, or layer2's 4 / 5 on the one-launch kernel; hmr_plan_configure)
  int wino_min_c = 128;
  // layer1's conv2 (64 channels) on the one-launch F(4x4,3x3) kernel when layer2's form is 4 or 5: 0 = none, 1 = block
  // layer1.0's only, 2 = also layer1.1's and layer1.2's, with or without conv3 behind them (POSERISK_WINO_LAYER1)
  int wino_layer1 = 1;
  bool fuse_downsample = true;  // first Bottlenecks: conv3 and the downsample branch as one dual-source GEMM
  bool fuse_conv3 = true;       // layer1 blocks 1, 2: conv2 (3x3, 64 channels) and conv3 in one kernel
  bool expand_regs = true;      // bf16 encoder: layer2's / layer3's conv3 + residual with the weights in registers (expand_res_bf16.hip)
  bool balanced = true;         // bf16 encoder: the evenly dealt persistent kernel where it pays (conv_bal_bf16.hip)
  int cus = 256;
  bool fuse_stem = true;        // conv1 + bn1 + relu + maxpool in one kernel (stem_pool_f32.hip / stem_pool_bf16.hip; needs stem_s2d)
  bool fuse_bottleneck = true;  // bf16 encoder, layer1 blocks 1, 2: the whole Bottleneck in one persistent kernel
  bool fuse_bottleneck2 = true; // bf16 encoder, layer2's plain blocks likewise (bottleneck128_bf16.hip)
  bool fuse_bottleneck3 = true; // bf16 encoder, layer3's plain blocks as one launch each when the batch fills the CUs (bottleneck256_bf16.hip)
  int b128_lead = 2;            // ... and the short chunk every second workgroup of that kernel opens with (A/B: POSERISK_B128_LEAD)
  bool stem_s2d = true;         // the 7x7 / stride-2 stem as a 4x4 / stride-1 convolution on the space-to-depth input
  bool regw = true;             // fp32: 1x1 / stride-1 layers with K = 128 / 256 on conv1x1_regw_f32 (weights in registers)
  int panel_max_k = 128;        // 1x1 / stride-1 expansions (conv3) with K up to this run as row panels (conv_fused.hip)
  int splitk = 1;               // fp32: split-K factor of the 7x7-map layers with 512 output channels; measured slower: off
  int fc_tiles = 0;             // POSERISK_FC_TILES=1: the regressor's FC layers on the 64x64 conv tiles (round 1's form)
  int fc_shape = 0;             // POSERISK_FC_SHAPE=<10 MT + NT>: output tiles per workgroup of fc_rows16_f32 (0 = by the batch; same bits)
  std::vector<ConvSpec> convs;
  FcSpec fc1x, fc1s, fc2, dec;
  float* init157 = nullptr;
  size_t wino_floats_per_frame = 0;
  int final_buf = 0;
  // A plain layer3 block as ONE launch (a frame per workgroup) beside its three ordinary launches `first .. first + 2` of the
  // plan: taken per sub-batch when its frames fill whole rounds of CUs (hmr_route), bit-identical either way.
  // convs[first].alt3 is its index here.
  struct FusedBlock {
    size_t first;
    ConvSpec blk;
  };
  std::vector<FusedBlock> fused3;
  // Where each block's output is complete (pr_hmr_encode_until): block 0 = the stem + max-pool, 1..16 = the Bottlenecks.
  // block_last[k] is the plan entry after which it is written (a whole-block spec, the last of a block's launches -- also
  // for the fused3 alternate, which spans the same three entries -- or a conv2 carrying conv3), block_buf[k] the buffer.
  static constexpr int kBlocks = 17;
  int block_last[kBlocks] = {};
  int block_buf[kBlocks] = {};
  // regressor workspaces (device, zero-filled)
  float* xf = nullptr;       // [B,2048]
  float* h_static = nullptr; // [B,1024]
  float* h1 = nullptr;       // [B,1024]
  float* h2 = nullptr;       // [B,1024]
  float* state = nullptr;    // [B,192]
};

size_t hmr_weight_floats();
// conv_form as pr_hmr_create accepts it (-1 default, 0, 2, 4, 5 or three digits of those)
bool hmr_conv_form_valid(int conv_form);
// Resolves the form (PR_CONV_FORM_DEFAULT -> the built-in default, moved by POSERISK_WINOGRAD) into plan->conv_form /
// stage_form and reads every POSERISK_* A/B switch of the plan from the environment -- once per handle.
void hmr_plan_configure(HmrPlan* plan, int precision, int conv_form, int max_batch);
// blob -> BN-folded packed weights (through `sink`) + the launch plan.  PR_OK or PR_ERR_INVALID (message set).
int hmr_plan_build(HmrPlan* plan, const float* blob, size_t n_floats, PlanSink& sink);

// A frame per workgroup (bottleneck256_bf16.hip) pays when the sub-batch's frames fill whole rounds of CUs: one round lasts as
// long for 1 frame as for `cus` (stand-alone at B=256: 137 us against 165 us for the three launches).
inline bool hmr_fused3_pays(int b, int cus) {
  const int rounds = (b + cus - 1) / cus;
  return b > 0 && (long)b * 100 >= (long)rounds * cus * 85;
}
// Sub-batch capacity for n concurrent sub-batches: a sub-batch is also the unit of one conv launch, whose tensors must stay
// under 2 GiB (the DMA kernels' out-of-range sentinel): 512 frames x 56x56x256 fp32 = 1.6 GB
inline int hmr_chunk_cap(int max_batch, int n_chunks) { return std::min(ceil_div(max_batch, n_chunks), 512); }
// Element counts of one sub-batch's workspaces: act[0] (the layout-changed input), act[1..5] (rotating feature maps), the
// Winograd V / M array, the split-K slab and tickets (0 = none).  bf16 maps hold the same elements in half the floats.
struct HmrChunkSizes {
  size_t act0_floats, act_floats, wino_floats, slab_floats, tickets;
};
HmrChunkSizes hmr_chunk_sizes(const HmrPlan& plan, int chunk_cap);
// Byte sizes of the tensors a plan entry reads and writes at B frames, from the entry's own dimensions: what the internal
// fence's tail mode places them by (hmr.hip `placed`; DESIGN.md "The internal fence").  A consumer must compute for its input
// what the producer computed for its output -- tests/native/fence_check.cc walks the plan and holds them to that.
// res is y's size, res3 is y3's.  A whole-Bottleneck spec is 1x1 / stride 1: x and y are the block's input and output.
inline size_t hmr_act_bytes(int precision, int B, int H, int W, int C) { return (size_t)B * H * W * C * (precision == 1 ? 2 : 4); }
struct ConvTensorBytes {
  size_t x = 0, y = 0, x2 = 0, y3 = 0;
};
inline ConvTensorBytes hmr_conv_tensor_bytes(const ConvSpec& c, int precision, int B) {
  ConvTensorBytes t;
  t.x = hmr_act_bytes(precision, B, c.H, c.W, c.Cin);
  t.y = hmr_act_bytes(precision, B, c.Ho(), c.Wo(), c.Cout);
  if (c.in2_buf >= 0) t.x2 = hmr_act_bytes(precision, B, c.H2, c.H2, c.Cin2);
  if (c.w3 && c.out3_buf >= 0) t.y3 = hmr_act_bytes(precision, B, c.Ho(), c.Wo(), c.N3);
  return t;
}
// Elements per frame of block k's output (pr_hmr_encode_until): the stem + max-pool, then layer1..layer4's blocks.
inline size_t hmr_block_frame_elems(int k) {
  if (k == 0) return (size_t)56 * 56 * 64;
  const int L = k <= 3 ? 0 : k <= 7 ? 1 : k <= 13 ? 2 : 3, hw = 56 >> L;
  return (size_t)hw * hw * (256 << L);
}
// Capacity in bytes of activation buffer `buf` (0 = the layout-changed input)
inline size_t hmr_act_capacity_bytes(const HmrChunkSizes& z, int buf) { return (buf == 0 ? z.act0_floats : z.act_floats) * sizeof(float); }
// V and M of a Winograd layer at B frames, in floats (conv_winograd_work_floats computes the same from its ConvProblem)
inline size_t hmr_wino_work_floats(const ConvSpec& c, int B) {
  const int m = c.wino_m;
  return (size_t)(m + 2) * (m + 2) * B * ((c.H + m - 1) / m) * ((c.W + m - 1) / m) * ((size_t)c.Cin + c.Cout);
}
// What one forward of B frames launches (pr_hmr_plan_counts): event brackets (a Winograd layer counts once) and how many
// of them are Winograd layers -- hmr_route walked over hmr_split_batch's sub-batches.
// `serial`: the passes run one after the other on the caller's stream (profile mode, or one sub-batch stream).
void hmr_plan_counts(const HmrPlan& plan, int B, int chunk_cap, int n_chunks, bool serial, int* conv_launches, int* winograd_layers);
// How pr_hmr_forward cuts B frames into sub-batches (the one place that decides it): serial passes of at most chunk_cap
// frames when one sub-batch runs at a time (also when a concurrent share would exceed chunk_cap), else n contiguous
// shares [c B / n, (c + 1) B / n) on the sub-batch streams.  Returns the number of sub-batches (<= 4096 / 1), their sizes
// in `sizes` (frames; room for max(n_chunks, ceil(B / chunk_cap)) entries), *concurrent = whether they run side by side.
int hmr_split_batch(int B, int chunk_cap, int n_chunks, bool serial, int* sizes, int max_sizes, bool* concurrent);

// ---- launch geometry -------------------------------------------------------------------------------------------
// What the launchers decide from a problem's SIZE alone -- the decisions that change with the batch -- as pure functions
// the launchers call, so that tests/native/launch_geometry.cc can enumerate them per batch size without a device
// (tests/test_launch_geometry.py: every geometry class that occurs up to 256 frames is run by a committed batch size).
// A/B switches of the conv launches.  Defaults are the measured best.  They are read from the environment ONCE per handle
// (conv_tuning_from_env, at pr_hmr_create; the stand-alone test entries read them per call) and travel in the
// ConvProblem, so two handles of one process can differ and nothing is latched per process.
struct ConvTuning {
  int force_cfg = -1;        // POSERISK_CONV_CFG=<index>: one tile configuration wherever it fits
  int tail = 1;              // POSERISK_CONV_TAIL=0: no quarter tiles for the remainder of a launch
  int tail_min_rounds = 2;   // POSERISK_TAIL_MIN_ROUNDS
  int tail_max_rem = 128;    // POSERISK_TAIL_MAX_REM
  int wino_vec = 2;          // POSERISK_WINO_VEC: channels per thread of the F(4x4) transform passes (2 or 4; same bits)
  int wino_bm = 64, wino_bn = 64;   // POSERISK_WINO_TILE=<BM>x<BN>: tile of the Winograd forms' grouped GEMM (A/B timing)
  int wino_regw = 1;         // POSERISK_WINO_REGW=0: the grouped GEMM of a Winograd layer with K = 128 / 256 on the tile kernel
                             // instead of the register-resident-weights kernel (conv_regw_f32.hip)
  int regw_per_cu = 2;       // POSERISK_REGW_PER_CU: persistent workgroups per CU of conv1x1_regw_f32 (A/B timing)
  int regw_wt = 0, regw_wnb = 0; // POSERISK_REGW_WT / POSERISK_REGW_WNB: the same for the grouped GEMMs of a Winograd layer
  int regw_t = 0, regw_nb = 0;   // POSERISK_REGW_T / POSERISK_REGW_NB: 16-pixel tiles and 64-channel blocks per unit of that kernel (0 = its defaults; same bits)
  int bal_stages = 4;        // POSERISK_BAL_STAGES=5: conv_bal_bf16's LDS ring of 5 stages (all 160 KB) instead of 4 (128 KB)
};

#if defined(__HIP__)
#define PR_HOST_DEVICE __host__ __device__
#else
#define PR_HOST_DEVICE
#endif

// conv_dma_launch's tile quantisation on 256 CUs: of `tiles` 64x64 tiles (split-K parts included) the ones beyond the last
// whole round of 256 run as quarter tiles -- four 32x32 work items each -- when the whole tiles run for at least
// `min_rounds` rounds and at most `max_rem` tiles remain, or when there are at most 64 tiles at all (every quarter then has a
// CU to itself).  grid = workgroups launched: n_full whole tiles, then the n_tail quarters padded to a multiple of 8 (one
// share per XCD).  `eligible`: the 64x64 / 4-wave tile without split-K, ConvTuning::tail on.
struct ConvTailSplit {
  int grid, n_full, n_tail;
};
inline ConvTailSplit conv_tail_split(int tiles, bool eligible, int min_rounds, int max_rem) {
  ConvTailSplit s{tiles, tiles, 0};
  if (!eligible) return s;
  const int rem = tiles % 256, rounds = tiles / 256;
  if ((rounds >= min_rounds && rem > 0 && rem <= max_rem) || tiles <= 64) {
    s.n_full = tiles - rem;
    s.n_tail = 4 * rem;
    s.grid = s.n_full + ceil_div(s.n_tail, 8) * 8;
  }
  return s;
}

// conv_regw_f32_launch: a unit is (NB blocks of 64 output channels, T tiles of 16 pixels) of one of `groups` GEMMs of M rows,
// unit u = (group * nblk + channel-block group) * pp + pixel group; `grid` persistent workgroups (at most per_cu per CU) take
// the contiguous runs [conv_regw_run_begin(wg), conv_regw_run_begin(wg + 1)).  t_knob / nb_knob: ConvTuning's pair for the
// problem's kind (regw_wt / regw_wnb when grouped, regw_t / regw_nb otherwise; 0 = the measured default).
struct RegwGeometry {
  int T, NB, pp, nblk, units, grid;
};
inline RegwGeometry conv_regw_geometry(int M, int Cin, int Cout, int groups, int t_knob, int nb_knob, int per_cu, int cus) {
  RegwGeometry g;
  const int nblk64 = Cout / 64;
  const bool grouped = groups > 1;       // the 36 GEMMs of a Winograd layer: their own pair of knobs
  g.NB = nb_knob > 0 ? nb_knob : (grouped ? 1 : 2);
  while (g.NB > 1 && (nblk64 % g.NB != 0 || (Cin == 256 && g.NB > 2))) g.NB >>= 1;
  g.T = t_knob > 0 ? t_knob : (grouped ? 2 : 1);
  if (g.T != 1 && g.T != 2) g.T = 2;
  g.pp = ceil_div(M, 16 * g.T);
  g.nblk = nblk64 / g.NB;
  g.units = g.pp * g.nblk * groups;
  g.grid = std::min(g.units, per_cu * cus);      // every workgroup an equal share of the units
  return g;
}
PR_HOST_DEVICE inline int conv_regw_run_begin(long wg, int units, long grid) { return (int)(wg * units / grid); }
// Whether some workgroup's run spans two channel blocks (u / pp changes inside it): it reloads its weights mid-run.
inline bool conv_regw_run_crosses(const RegwGeometry& g) {
  for (int wg = 0; wg < g.grid; ++wg) {
    const int u0 = conv_regw_run_begin(wg, g.units, g.grid), u1 = conv_regw_run_begin(wg + 1, g.units, g.grid);
    if (u1 > u0 && (u1 - 1) / g.pp != u0 / g.pp) return true;
  }
  return false;
}

// conv_panel_launch: column parts per 64-row panel -- enough work items to balance 256 CUs (about 6 per CU where the layer allows)
inline int conv_panel_nsplit(int panels, int nchunks) {
  int nsplit = 1;
  while (nsplit * 2 <= nchunks && nchunks % (nsplit * 2) == 0 && panels * nsplit < 1536) nsplit *= 2;
  return nsplit;
}

// ---- which kernel --------------------------------------------------------------------------------------------------
// The tile configurations conv_launch takes an index into.  Retired indices stay reserved (conv_launch refuses them by name)
// so that the live ones keep their numbers in profiles/ and scripts/tune_conv.py.
struct ConvTileCfg {
  int BM, BN, threads;
  const char* name;
  int blocks_per_cu;   // LDS-limited residency
  bool live = true;    // false: retired, the index is kept and refused
};
int conv_num_tile_cfgs();
const ConvTileCfg* conv_tile_cfg(int cfg);      // null outside 0 .. conv_num_tile_cfgs() - 1
int conv_pick_tile_cfg(const ConvShape& s, const ConvTuning& tune);      // chip-filling heuristic
// What conv_bal_bf16_launch / conv_regw_f32_launch take, and the measured rule for the balanced kernel over the tile kernel
bool conv_bal_bf16_fits(const ConvShape& s);
bool conv_bal_bf16_pays(const ConvShape& s, int cus);
bool conv_regw_f32_fits(const ConvShape& s);

// Which kernel carries plan entry `ci` when the sub-batch has `b` frames, in this order of precedence: layer3's whole-block
// alternate where hmr_fused3_pays; the stem with its max-pool; a whole-Bottleneck spec; layer1's one-launch Winograd; a
// three-launch Winograd layer; else conv_launch with the entry's own cfg or the picked tile, balanced where conv_bal_bf16_pays.
enum class HmrKernel { StemPool, Bottleneck, Wino64, Winograd, Fused3, Tile, Panel, RegW, Expand, Balanced };
struct HmrRoute {
  HmrKernel kernel;
  int cfg;                // what conv_launch gets (Fused3 .. Balanced), else -1
  const ConvSpec* spec;   // what is launched: the entry, or FusedBlock::blk for layer3's alternate
  int span;               // plan entries the launch covers: 3 for that alternate, else 1
  int layer;              // the profile reports it under this convolution index
};
HmrRoute hmr_route(const HmrPlan& plan, const ConvTuning& tune, size_t ci, int b);

}  // namespace pr
