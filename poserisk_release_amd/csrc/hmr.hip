// pr_hmr: SPIN HMR (ResNet-50 encoder + 3-iteration regressor + rot6d->rotmat) on gfx950.
// Replaces models.hmr / spin_model(batch)  (lib/core/base.py:81-84, :220).
//
// The host side that needs no device -- parsing the canonical weight blob (include/poserisk_hip.h), folding eval-mode
// BatchNorm into the convolutions in double, packing weights for every kernel family, the 53-conv execution plan over NHWC
// activation buffers, the regressor's fc1 split into its constant part (pooled features, computed once) and its state part
// (157 inputs, recomputed per iteration), and which kernel carries which plan entry at which batch (hmr_route) -- is
// host_plan.cc (plain C++, also built under ASan + UBSan by tests/native).
// Here: device memory, workspaces, streams, and the launch sequence, which executes hmr_route's answer entry by entry.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "conv_igemm.h"
#include "fence.h"
#include "frame_kernels.h"

struct pr_hmr : pr::HmrPlan {
  // settings, the 53-convolution plan, packed-weight pointers and regressor workspaces: pr::HmrPlan (host_plan.h, built by
  // hmr_plan_build -- device-free code that tests/native runs under ASan + UBSan); what follows is the device state
  int device = 0;
  pr::ConvTuning tune;          // tile-choice / quarter-tile switches of the conv launches (read once, at create)
  float* split_slab[8] = {};      // per sub-batch chunk (kMaxChunks)
  int* split_tickets[8] = {};
  std::vector<float*> dev_allocs;
  // activation buffers per frame chunk: 0 = NHWC4 input, 1..5 = rotating feature maps.
  // The batch is cut into n_chunks contiguous sub-batches that run the encoder on their own
  // HIP streams (frames are independent).  Measured on MI355X at B=64 this lock-step form is SLOWER
  // than one stream (sub-batch kernels are smaller and all streams run the same layer at once), so the
  // default is 1; what does pay is whole batches in flight on different streams, which the caller
  // drives (pipeline.FramePipeline lanes).  Kept because it is bit-identical and lets a batch exceed
  // one sub-batch's workspace.
  static constexpr int kMaxChunks = pr::kHmrMaxChunks;
  int n_chunks = 1;
  int chunk_cap = 0;
  float* act[kMaxChunks][6] = {};
  float* wino_work[kMaxChunks] = {};  // V and M of the Winograd layers (conv_winograd.hip)
  hipStream_t streams[kMaxChunks] = {};
  hipEvent_t ev_fork = nullptr;
  hipEvent_t ev_join[kMaxChunks] = {};
  std::vector<float*> act_allocs;
  // the internal fence (POSERISK_FENCE, read at create and at set_streams; fence.h): 0 = off, 1 = head, 2 = tail.  In tail
  // mode every tensor in act / wino_work / split_slab ends on its buffer's last byte (`placed` below); `sizes` is what those
  // buffers hold.  fence_bad: a tensor did not fit its buffer or its size was no multiple of 256 bytes -- the forward fails.
  int fence = 0;
  pr::HmrChunkSizes sizes{};
  bool fence_bad = false;
  // profiling
  bool profile = false;
  std::vector<float> prof_ms;
  std::vector<int> prof_n;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> pending;
  std::vector<int> pending_layer;
};

namespace pr {
namespace {

// hmr_plan_build's constants land in device memory, owned by the handle
struct DeviceSink : PlanSink {
  pr_hmr* h;
  explicit DeviceSink(pr_hmr* handle) : h(handle) {}
  int upload(const void* host, size_t bytes, float** out) override {
    float* d = nullptr;
    PR_TRY(device_alloc((void**)&d, std::max<size_t>(bytes, 16), h->fence, 0, "plan constant %zu", h->dev_allocs.size()));
    h->dev_allocs.push_back(d);
    PR_HIP(hipMemcpy(d, host, bytes, hipMemcpyHostToDevice));
    *out = d;
    return PR_OK;
  }
  int zeros(size_t bytes, float** out) override {
    float* d = nullptr;
    PR_TRY(device_alloc((void**)&d, std::max<size_t>(bytes, 16), h->fence, 0, "plan workspace %zu", h->dev_allocs.size()));
    h->dev_allocs.push_back(d);
    PR_HIP(hipMemset(d, 0, std::max<size_t>(bytes, 16)));
    *out = d;
    return PR_OK;
  }
};

// (Re)allocate the activation buffers for n sub-batches and create their streams / events.
int set_chunks(pr_hmr* h, int n) {
  PR_REQUIRE(n >= 1 && n <= pr_hmr::kMaxChunks, "hmr: stream count %d out of range 1..%d", n, pr_hmr::kMaxChunks);
  PR_HIP(hipDeviceSynchronize());
  PR_REQUIRE(!h->convs.empty() && h->convs[0].in_buf == 0, "hmr: the plan's first entry reads the layout-changed input");
  for (float* p : h->act_allocs) device_free(p);
  h->act_allocs.clear();
  h->n_chunks = n;
  // a sub-batch is also the unit of one conv launch, whose tensors must stay under 2 GiB (the DMA kernel's
  // out-of-range sentinel): 512 frames x 56x56x256 fp32 = 1.6 GB
  h->chunk_cap = hmr_chunk_cap(h->max_batch, n);
  const HmrChunkSizes z = hmr_chunk_sizes(*h, h->chunk_cap);   // element counts per sub-batch (host_plan.cc)
  h->sizes = z;
  // a guard of the internal fence: one frame of the largest tensor the buffer holds
  const size_t cb = (size_t)h->chunk_cap;
  for (int c = 0; c < n; ++c) {
    for (int i = 0; i <= 5; ++i) {
      float* d = nullptr;
      const size_t floats = i == 0 ? z.act0_floats : z.act_floats;
      PR_TRY(device_alloc((void**)&d, floats * sizeof(float), h->fence, floats * sizeof(float) / cb, "act[%d][%d]", c, i));
      h->act_allocs.push_back(d);
      h->act[c][i] = d;
    }
    if (z.wino_floats) {
      float* d = nullptr;
      PR_TRY(device_alloc((void**)&d, z.wino_floats * sizeof(float), h->fence, h->wino_floats_per_frame * sizeof(float), "wino_work[%d]", c));
      h->act_allocs.push_back(d);
      h->wino_work[c] = d;
    }
    if (z.slab_floats) {
      float* d = nullptr;
      PR_TRY(device_alloc((void**)&d, z.slab_floats * sizeof(float), h->fence, z.slab_floats * sizeof(float) / cb, "split_slab[%d]", c));
      h->act_allocs.push_back(d);
      h->split_slab[c] = d;
      PR_TRY(device_alloc((void**)&d, z.tickets * sizeof(int), h->fence, 0, "split_tickets[%d]", c));
      h->act_allocs.push_back(d);
      h->split_tickets[c] = reinterpret_cast<int*>(d);
    }
    if (n > 1 && !h->streams[c]) PR_HIP(hipStreamCreateWithFlags(&h->streams[c], hipStreamNonBlocking));
    if (n > 1 && !h->ev_join[c]) PR_HIP(hipEventCreateWithFlags(&h->ev_join[c], hipEventDisableTiming));
  }
  if (n > 1 && !h->ev_fork) PR_HIP(hipEventCreateWithFlags(&h->ev_fork, hipEventDisableTiming));
  return PR_OK;
}

// Where a tensor of `bytes` lies in one of the buffers that are sized as a maximum over layers and over the batch: on the
// buffer's first byte, or -- internal fence in tail mode -- ending on its last, so that the guard behind the buffer is sharp
// for every layer at every B.  Producer and consumer of a tensor compute the same place from the same dimensions.
template <typename T>
T* placed(pr_hmr* h, T* base, size_t capacity_bytes, size_t bytes) {
  if (h->fence != 2 || !base) return base;
  bool ok = true;
  const size_t off = fence_tail_offset(capacity_bytes, bytes, &ok);
  if (!ok && !h->fence_bad) {
    h->fence_bad = true;
    set_error("hmr: internal fence: a tensor of %zu bytes in a buffer of %zu (it must fit and be a multiple of 256 bytes)", bytes,
              capacity_bytes);
  }
  return reinterpret_cast<T*>(reinterpret_cast<char*>(base) + off);
}
// A tensor of `bytes` in activation buffer `buf`; act_at: the tensor [B, H, W, C] in the handle's precision
float* act_placed(pr_hmr* h, int chunk, int buf, size_t bytes) {
  return placed(h, h->act[chunk][buf], hmr_act_capacity_bytes(h->sizes, buf), bytes);
}
float* act_at(pr_hmr* h, int chunk, int buf, int B, int H, int W, int C) {
  return act_placed(h, chunk, buf, hmr_act_bytes(h->precision, B, H, W, C));
}
// The encoder's input after the layout change, as the stem (plan entry 0) reads it
float* stem_in_at(pr_hmr* h, int chunk, int B) {
  return act_placed(h, chunk, 0, hmr_conv_tensor_bytes(h->convs[0], h->precision, B).x);
}
// V and M of a Winograd layer at this B (hmr_plan_build's wino_floats_per_frame is the maximum of the same product per frame)
float* wino_work_at(pr_hmr* h, int chunk, const ConvSpec& c, int B) {
  return placed(h, h->wino_work[chunk], h->sizes.wino_floats * sizeof(float), hmr_wino_work_floats(c, B) * sizeof(float));
}

ConvProblem conv_problem(pr_hmr* h, const ConvSpec& c, int chunk, int B) {
  ConvProblem p;
  const ConvTensorBytes t = hmr_conv_tensor_bytes(c, h->precision, B);
  p.x = act_placed(h, chunk, c.in_buf, t.x);
  p.w = c.w;
  p.bias = c.bias;
  p.res = c.res_buf >= 0 ? act_placed(h, chunk, c.res_buf, t.y) : nullptr;
  p.y = act_placed(h, chunk, c.out_buf, t.y);
  p.B = B; p.H = c.H; p.W = c.W; p.Cin = c.Cin; p.Ho = c.Ho(); p.Wo = c.Wo(); p.Cout = c.Cout;
  p.KH = p.KW = c.k; p.stride = c.stride; p.pad = c.pad; p.relu = c.relu;
  p.precision = h->precision;
  p.tune = h->tune;
  if (c.in2_buf >= 0) {
    p.x2 = act_placed(h, chunk, c.in2_buf, t.x2);
    p.H2 = p.W2 = c.H2; p.Cin2 = c.Cin2; p.stride2 = c.stride2;
  }
  if (c.splitk > 1) {
    p.splitk = c.splitk;
    // one 64x64 fp32 partial tile per K part (hmr_chunk_sizes); the tickets, one int a tile, stay on their buffer's first
    // byte in both modes: their size is no multiple of 256 bytes
    const size_t tiles = (size_t)ceil_div(B * c.Ho() * c.Wo(), 64) * (c.Cout / 64);
    p.split_slab = placed(h, h->split_slab[chunk], h->sizes.slab_floats * sizeof(float), tiles * c.splitk * 4096 * sizeof(float));
    p.split_tickets = h->split_tickets[chunk];
  }
  if (c.w3 && c.out3_buf >= 0) {
    p.w3 = c.w3; p.bias3 = c.bias3; p.N3 = c.N3; p.relu3 = 1;
    p.res3 = c.res3_buf >= 0 ? act_placed(h, chunk, c.res3_buf, t.y3) : nullptr;
    p.y3 = act_placed(h, chunk, c.out3_buf, t.y3);
  }
  return p;
}

int fc_launch(const pr_hmr* h, const FcSpec& fc, const float* x, const float* res, float* y, int B, bool use_bias,
              hipStream_t s) {
  // A/B switch (pr_hmr::fc_tiles): the layer on the 64x64 conv tiles (round 1's form) instead of fc_regressor.hip
  if (!h->fc_tiles) return launch_fc_rows16(x, fc.w, use_bias ? fc.bias : nullptr, res, y, B, fc.N, fc.K, s, h->fc_shape);
  ConvProblem p;
  p.x = x; p.w = fc.w; p.bias = use_bias ? fc.bias : nullptr; p.res = res; p.y = y;
  p.B = B; p.H = p.W = p.Ho = p.Wo = 1; p.Cin = fc.K; p.Cout = fc.N;
  p.KH = p.KW = 1; p.stride = 1; p.pad = 0; p.relu = 0;
  p.tune = h->tune;
  return conv_launch(p, conv_pick_tile_cfg(p.shape(), p.tune), s);
}


// One sub-batch of the encoder: where it reads, where it writes, which stream it runs on.
struct ChunkRun {
  int chunk;
  const float* x;
  int b;
  float* xf_out;
  hipStream_t s;
  void* tap = nullptr;   // encode_until: where this sub-batch's frames of the tapped block go
};


// A whole Bottleneck (a bneck_planes entry, or layer3's alternate) is launched from its spec's own fields: no ConvProblem.
// lead_tiles is bottleneck128_bf16's alone; the other two kernels ignore it.
BottleneckProblem bottleneck_problem(pr_hmr* h, const ConvSpec& c, int chunk, int B) {
  BottleneckProblem bp;
  const ConvTensorBytes t = hmr_conv_tensor_bytes(c, h->precision, B);
  bp.x = act_placed(h, chunk, c.in_buf, t.x); bp.y = act_placed(h, chunk, c.out_buf, t.y);
  bp.w1 = c.w; bp.w2 = c.w2b; bp.w3 = c.w3; bp.b1 = c.bias; bp.b2 = c.bias2b; bp.b3 = c.bias3;
  bp.B = B; bp.H = c.H; bp.W = c.W; bp.planes = c.bneck_planes; bp.first = c.bneck_first;
  bp.lead_tiles = h->b128_lead;
  return bp;
}

// One launch of the plan; in profile mode bracketed by events that pr_hmr_profile_read adds up under `layer`
template <typename Launch>
int timed(pr_hmr* h, int layer, hipStream_t s, Launch launch) {
  if (!h->profile) return launch();
  hipEvent_t e0, e1;
  PR_HIP(hipEventCreate(&e0));
  PR_HIP(hipEventCreate(&e1));
  PR_HIP(hipEventRecord(e0, s));
  PR_TRY(launch());
  PR_HIP(hipEventRecord(e1, s));
  h->pending.emplace_back(e0, e1);
  h->pending_layer.push_back(layer);
  return PR_OK;
}

// Encoder over n sub-batches: layout change, 53 convs, max-pool, global average pool -> xf[b,2048].
// Launches are issued layer by layer across the sub-batches so that all streams advance together
// (issuing one whole sub-batch after another would stagger them by the host's enqueue time).
// Which kernel carries an entry for a sub-batch, and how many entries it covers: hmr_route (host_plan.cc); this executes it.
// stop_block >= 0 (pr_hmr_encode_until): after the plan entry that completes that block, each sub-batch's copy of it goes to
// its run's `tap` and nothing further is launched.
int encode_chunks(pr_hmr* h, const ChunkRun* runs, int n, int stop_block = -1) {
  const bool bf = h->precision == 1;
  for (int i = 0; i < n; ++i) {
    if (h->stem_s2d) {
      if (bf) PR_TRY(launch_nchw3_to_s2d16_bf16(runs[i].x, stem_in_at(h, runs[i].chunk, runs[i].b), runs[i].b, kImg, kImg, runs[i].s));
      else PR_TRY(launch_nchw3_to_s2d12(runs[i].x, stem_in_at(h, runs[i].chunk, runs[i].b), runs[i].b, kImg, kImg, runs[i].s));
    } else {
      if (bf) PR_TRY(launch_nchw3_to_nhwc8_bf16(runs[i].x, stem_in_at(h, runs[i].chunk, runs[i].b), runs[i].b, kImg, kImg, runs[i].s));
      else PR_TRY(launch_nchw3_to_nhwc4(runs[i].x, stem_in_at(h, runs[i].chunk, runs[i].b), runs[i].b, kImg, kImg, runs[i].s));
    }
  }
  size_t next[pr_hmr::kMaxChunks] = {};      // per sub-batch: the first entry no launch has covered yet
  for (size_t ci = 0; ci < h->convs.size(); ++ci) {
    for (int i = 0; i < n; ++i) {
      const ChunkRun& r = runs[i];
      if (ci < next[i]) continue;
      const HmrRoute rt = hmr_route(*h, h->tune, ci, r.b);
      const ConvSpec& c = *rt.spec;
      next[i] = ci + rt.span;
      PR_TRY(timed(h, rt.layer, r.s, [&]() -> int {
        switch (rt.kernel) {
          case HmrKernel::StemPool: {
            float* const y = act_at(h, r.chunk, 2, r.b, 56, 56, 64);
            if (bf) return stem_pool_bf16_launch(stem_in_at(h, r.chunk, r.b), c.w, c.bias, y, r.b, kImg / 2, r.s);
            return stem_pool_f32_launch(stem_in_at(h, r.chunk, r.b), c.w, c.bias, y, r.b, r.s);
          }
          case HmrKernel::Bottleneck: return bottleneck_bf16_launch(bottleneck_problem(h, c, r.chunk, r.b), r.s);
          case HmrKernel::Wino64: return conv_wino64_launch(conv_problem(h, c, r.chunk, r.b), c.u1, h->stage_form[0], r.s);
          case HmrKernel::Winograd:
            return conv_winograd_launch(conv_problem(h, c, r.chunk, r.b), c.u, wino_work_at(h, r.chunk, c, r.b), c.wino_form, r.s);
          case HmrKernel::Fused3: case HmrKernel::Tile: case HmrKernel::Panel: case HmrKernel::RegW: case HmrKernel::Expand:
          case HmrKernel::Balanced: return conv_launch(conv_problem(h, c, r.chunk, r.b), rt.cfg, r.s);
        }
        return PR_ERR_INVALID;
      }));
      if (ci == 0 && rt.kernel != HmrKernel::StemPool) {
        float* const pool_in = act_at(h, r.chunk, 1, r.b, 112, 112, 64);
        float* const pool_out = act_at(h, r.chunk, 2, r.b, 56, 56, 64);
        if (bf) PR_TRY(launch_maxpool_bf16(pool_in, pool_out, r.b, 112, 112, 64, r.s));
        else PR_TRY(launch_maxpool(pool_in, pool_out, r.b, 112, 112, 64, r.s));
      }
    }
    if (stop_block >= 0 && ci == (size_t)h->block_last[stop_block]) {
      const size_t frame_bytes = hmr_block_frame_elems(stop_block) * (bf ? 2 : 4);
      for (int i = 0; i < n; ++i)
        PR_HIP(hipMemcpyAsync(runs[i].tap,
                              act_placed(h, runs[i].chunk, h->block_buf[stop_block], runs[i].b * frame_bytes),
                              runs[i].b * frame_bytes, hipMemcpyDeviceToDevice, runs[i].s));
      return PR_OK;
    }
  }
  for (int i = 0; i < n; ++i) {
    float* const last = act_at(h, runs[i].chunk, h->final_buf, runs[i].b, 7, 7, 2048);
    if (bf) PR_TRY(launch_avgpool_bf16(last, runs[i].xf_out, runs[i].b, 49, 2048, runs[i].s));
    else PR_TRY(launch_avgpool(last, runs[i].xf_out, runs[i].b, 49, 2048, runs[i].s));
  }
  return PR_OK;
}

// The internal fence's names of what hmr_plan_build uploaded: by the network's convolution index (ConvSpec::layer) or the
// regressor's part.  (The sink sees bytes only; the plan knows whose they are once it is built.)
void name_plan_constants(pr_hmr* h) {
  auto conv = [](const ConvSpec& c, const char* kind) {
    fence_rename(c.w, "%s %d weights", kind, c.layer);
    fence_rename(c.bias, "%s %d bias", kind, c.layer);
    fence_rename(c.u, "%s %d u", kind, c.layer);
    fence_rename(c.u1, "%s %d u1", kind, c.layer);
    fence_rename(c.w3, "%s %d conv3 weights", kind, c.layer);
    fence_rename(c.bias3, "%s %d conv3 bias", kind, c.layer);
    fence_rename(c.w2b, "%s %d conv2 weights", kind, c.layer);
    fence_rename(c.bias2b, "%s %d conv2 bias", kind, c.layer);
  };
  for (const ConvSpec& c : h->convs) conv(c, c.bneck_planes ? "block" : "conv");
  for (const pr::HmrPlan::FusedBlock& fb : h->fused3) conv(fb.blk, "block256");
  const FcSpec* fcs[4] = {&h->fc1x, &h->fc1s, &h->fc2, &h->dec};
  const char* fc_names[4] = {"fc1x", "fc1s", "fc2", "dec"};
  for (int i = 0; i < 4; ++i) {
    fence_rename(fcs[i]->w, "%s weights", fc_names[i]);
    fence_rename(fcs[i]->bias, "%s bias", fc_names[i]);
  }
  fence_rename(h->init157, "init157");
  fence_rename(h->xf, "xf");
  fence_rename(h->h_static, "h_static");
  fence_rename(h->h1, "h1");
  fence_rename(h->h2, "h2");
  fence_rename(h->state, "state");
}

}  // namespace
}  // namespace pr

extern "C" {

size_t pr_hmr_weight_floats(void) { return pr::hmr_weight_floats(); }
int pr_hmr_num_conv_layers(void) { return pr::kNumConv; }

int pr_hmr_create(int device, const float* weights_host, size_t n_floats, int max_batch, int precision,
                  int conv_form, pr_hmr_t** out) {
  using namespace pr;
  PR_REQUIRE(out && weights_host, "pr_hmr_create: null argument");
  PR_REQUIRE(max_batch > 0 && max_batch <= 4096, "pr_hmr_create: max_batch %d out of range", max_batch);
  PR_REQUIRE(precision == 0 || precision == 1, "pr_hmr_create: precision %d unknown (0 = fp32, 1 = bf16 encoder)", precision);
  PR_REQUIRE(hmr_conv_form_valid(conv_form),
             "pr_hmr_create: conv_form %d unknown (-1 default, 0 direct, 2 F(2x2,3x3), 4 F(4x4,3x3), 5 F(4x4,3x3) on the "
             "points 0, +-11/16, +-3/2, or three digits of those for layer2 / layer3 / layer4)", conv_form);
  PR_REQUIRE(n_floats == hmr_weight_floats(), "pr_hmr_create: blob has %zu floats, expected %zu", n_floats,
             hmr_weight_floats());
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
    set_error("pr_hmr_create: no HIP device visible");
    return PR_ERR_NO_DEVICE;
  }
  PR_REQUIRE(device >= 0 && device < ndev, "pr_hmr_create: device %d of %d", device, ndev);
  DeviceGuard g(device);
  PR_TRY(refuse_under_declared_capture("pr_hmr_create"));
  std::unique_ptr<pr_hmr> h(new pr_hmr);
  h->device = device;
  // the conv form and every POSERISK_* A/B switch: read here, once per handle (nothing is latched per process)
  hmr_plan_configure(h.get(), precision, conv_form, max_batch);
  h->tune = conv_tuning_from_env();
  h->fence = fence_mode_from_env();
  (void)hipDeviceGetAttribute(&h->cus, hipDeviceAttributeMultiprocessorCount, h->device);
  DeviceSink sink(h.get());
  int st = hmr_plan_build(h.get(), weights_host, n_floats, sink);
  h->prof_ms.assign(kNumConv, 0.f);
  h->prof_n.assign(kNumConv, 0);
  if (st == PR_OK && h->fence) name_plan_constants(h.get());
  if (st == PR_OK) {
    int n = 1;  // sub-batch streams: 1 unless POSERISK_HMR_STREAMS / pr_hmr_set_streams ask for more
    if (const char* e = getenv("POSERISK_HMR_STREAMS")) n = atoi(e);
    n = std::max(1, std::min(n, (int)pr_hmr::kMaxChunks));
    st = set_chunks(h.get(), std::min(n, max_batch));
  }
  if (st != PR_OK) {
    for (float* p : h->dev_allocs) device_free(p);
    for (float* p : h->act_allocs) device_free(p);
    return st;
  }
  *out = h.release();
  return PR_OK;
}

int pr_hmr_destroy(pr_hmr_t* h) {
  if (!h) return PR_OK;
  pr::DeviceGuard g(h->device);
  PR_TRY(pr::refuse_under_declared_capture("pr_hmr_destroy"));   // the handle stays valid: destroy it after the capture
  for (auto& pe : h->pending) {
    (void)hipEventDestroy(pe.first);
    (void)hipEventDestroy(pe.second);
  }
  for (float* p : h->dev_allocs) pr::device_free(p);
  for (float* p : h->act_allocs) pr::device_free(p);
  for (int c = 0; c < pr_hmr::kMaxChunks; ++c) {
    if (h->streams[c]) (void)hipStreamDestroy(h->streams[c]);
    if (h->ev_join[c]) (void)hipEventDestroy(h->ev_join[c]);
  }
  if (h->ev_fork) (void)hipEventDestroy(h->ev_fork);
  delete h;
  return PR_OK;
}

int pr_hmr_set_concurrency(pr_hmr_t* h, int n_in_flight) {
  PR_REQUIRE(h, "pr_hmr_set_concurrency: null handle");
  PR_REQUIRE(n_in_flight >= 1, "pr_hmr_set_concurrency: %d handles in flight", n_in_flight);
  if (!getenv("POSERISK_REGW_PER_CU")) h->tune.regw_per_cu = n_in_flight >= 2 ? 1 : 2;   // the env is the A/B override
  return PR_OK;
}

int pr_hmr_set_streams(pr_hmr_t* h, int n_streams) {
  PR_REQUIRE(h, "pr_hmr_set_streams: null handle");
  pr::DeviceGuard g(h->device);
  PR_TRY(pr::refuse_under_declared_capture("pr_hmr_set_streams"));
  h->fence = pr::fence_mode_from_env();   // the buffers allocated below are the ones `placed` places tensors in
  return pr::set_chunks(h, std::min(n_streams, h->max_batch));
}

}  // extern "C"

namespace pr {
namespace {
// The encoder of pr_hmr_forward (stop_block < 0) or its early exit of pr_hmr_encode_until, on the same sub-batch split.
int encode_batch(pr_hmr_t* h, const float* x_dev, int B, hipStream_t s, int stop_block, void* tap) {
  // Profiling runs serially on the caller's stream so that each conv's event bracket is its own time.  The split is
  // hmr_split_batch's (host_plan.cc), which pr_hmr_plan_counts walks too.
  int sizes[4096];
  bool concurrent = false;
  const int nsub = hmr_split_batch(B, h->chunk_cap, h->n_chunks, h->profile != 0, sizes, 4096, &concurrent);
  const size_t frame = (size_t)3 * kImg * kImg;
  const size_t tap_frame = stop_block >= 0 ? hmr_block_frame_elems(stop_block) * (h->precision == 1 ? 2 : 4) : 0;
  auto tap_at = [&](int b0) { return tap ? (void*)((char*)tap + (size_t)b0 * tap_frame) : nullptr; };
  if (!concurrent) {
    // one sub-batch at a time on the caller's stream (more than one pass if B exceeds a chunk's buffers)
    for (int i = 0, b0 = 0; i < nsub; b0 += sizes[i], ++i) {
      ChunkRun r{0, x_dev + b0 * frame, sizes[i], h->xf + (size_t)b0 * 2048, s, tap_at(b0)};
      PR_TRY(encode_chunks(h, &r, 1, stop_block));
    }
    PR_REQUIRE(!h->fence_bad, "%s", pr_last_error());
  } else {
    const int nch = nsub;
    ChunkRun runs[pr_hmr::kMaxChunks];
    PR_HIP(hipEventRecord(h->ev_fork, s));
    for (int c = 0, b0 = 0; c < nch; b0 += sizes[c], ++c) {
      runs[c] = ChunkRun{c, x_dev + b0 * frame, sizes[c], h->xf + (size_t)b0 * 2048, h->streams[c], tap_at(b0)};
      PR_HIP(hipStreamWaitEvent(h->streams[c], h->ev_fork, 0));
    }
    PR_TRY(encode_chunks(h, runs, nch, stop_block));
    PR_REQUIRE(!h->fence_bad, "%s", pr_last_error());
    for (int c = 0; c < nch; ++c) {
      PR_HIP(hipEventRecord(h->ev_join[c], h->streams[c]));
      PR_HIP(hipStreamWaitEvent(s, h->ev_join[c], 0));
    }
  }
  return PR_OK;
}

// The regressor of pr_hmr_forward, launch by launch, stopped after launch `last` (10 = all of it; pr_hmr_regress_until
// stops earlier): h_static = xf*W1x^T + b1 once; 3 x { h1 = state*W1s^T + h_static; h2 = h1*W2^T + b2;
// state += h2*Wdec^T + bdec }.  Launch 0 = the state's initial value, 1 = fc1x, 2 + 3 i / 3 + 3 i / 4 + 3 i = iteration i's
// fc1s / fc2 / dec.
int regress_steps(pr_hmr_t* h, const float* xf, int B, int last, hipStream_t s) {
  PR_TRY(launch_state_init(h->init157, h->state, B, s));
  if (last < 1) return PR_OK;
  PR_TRY(fc_launch(h, h->fc1x, xf, nullptr, h->h_static, B, true, s));
  for (int it = 0; it < 3; ++it) {
    if (last < 2 + 3 * it) return PR_OK;
    PR_TRY(fc_launch(h, h->fc1s, h->state, h->h_static, h->h1, B, false, s));
    if (last < 3 + 3 * it) return PR_OK;
    PR_TRY(fc_launch(h, h->fc2, h->h1, nullptr, h->h2, B, true, s));
    if (last < 4 + 3 * it) return PR_OK;
    PR_TRY(fc_launch(h, h->dec, h->h2, h->state, h->state, B, true, s));
  }
  return PR_OK;
}
}  // namespace
}  // namespace pr

extern "C" {

int pr_hmr_forward(pr_hmr_t* h, const float* x_dev, int B, float* rotmat_dev, float* betas_dev,
                   float* cam_dev, float* xf_dev, float* pose6d_dev, void* stream) {
  using namespace pr;
  PR_REQUIRE(B >= 0, "pr_hmr_forward: negative batch");
  if (B == 0) return PR_OK;
  PR_REQUIRE(h && x_dev, "pr_hmr_forward: null argument");
  if (B > h->max_batch) {
    set_error("pr_hmr_forward: batch %d exceeds max_batch %d", B, h->max_batch);
    return PR_ERR_CAPACITY;
  }
  hipStream_t s = (hipStream_t)stream;
  PR_TRY(encode_batch(h, x_dev, B, s, -1, nullptr));
  if (xf_dev) PR_HIP(hipMemcpyAsync(xf_dev, h->xf, (size_t)B * 2048 * sizeof(float), hipMemcpyDeviceToDevice, s));
  if (!rotmat_dev && !betas_dev && !cam_dev && !pose6d_dev) return PR_OK;
  PR_TRY(regress_steps(h, h->xf, B, 10, s));
  PR_TRY(launch_regressor_finalize(h->state, rotmat_dev, betas_dev, cam_dev, pose6d_dev, B, s));
  return PR_OK;
}

int pr_hmr_encode_until(pr_hmr_t* h, const float* x_dev, int B, int block, void* act_dev, void* stream) {
  using namespace pr;
  PR_REQUIRE(B >= 1, "pr_hmr_encode_until: batch %d out of range", B);
  PR_REQUIRE(block >= 0 && block < HmrPlan::kBlocks, "pr_hmr_encode_until: block %d out of range 0..%d", block,
             HmrPlan::kBlocks - 1);
  PR_REQUIRE(h && x_dev && act_dev, "pr_hmr_encode_until: null argument");
  PR_REQUIRE(B <= h->max_batch, "pr_hmr_encode_until: batch %d out of range 1..%d", B, h->max_batch);
  hipStream_t s = (hipStream_t)stream;
  PR_TRY(refuse_if_capturing(s, "pr_hmr_encode_until"));   // a test entry: never part of a captured forward
  return encode_batch(h, x_dev, B, s, block, act_dev);
}

int pr_hmr_regress_until(pr_hmr_t* h, const float* xf_dev, int B, int step, float* out_dev, void* stream) {
  using namespace pr;
  PR_REQUIRE(B >= 1, "pr_hmr_regress_until: batch %d out of range", B);
  PR_REQUIRE(step >= 0 && step <= 10, "pr_hmr_regress_until: step %d out of range 0..10", step);
  PR_REQUIRE(h && xf_dev && out_dev, "pr_hmr_regress_until: null argument");
  PR_REQUIRE(B <= h->max_batch, "pr_hmr_regress_until: batch %d out of range 1..%d", B, h->max_batch);
  hipStream_t s = (hipStream_t)stream;
  PR_TRY(refuse_if_capturing(s, "pr_hmr_regress_until"));   // a test entry: never part of a captured forward
  PR_TRY(regress_steps(h, xf_dev, B, step, s));
  // what launch `step` wrote: the state (init, dec), h_static (fc1x), h1 (fc1s) or h2 (fc2)
  const int phase = step < 2 ? step : 2 + (step - 2) % 3;
  const float* src = phase == 0 || phase == 4 ? h->state : phase == 1 ? h->h_static : phase == 2 ? h->h1 : h->h2;
  const size_t cols = phase == 0 || phase == 4 ? kStateStride : 1024;
  PR_HIP(hipMemcpyAsync(out_dev, src, (size_t)B * cols * sizeof(float), hipMemcpyDeviceToDevice, s));
  return PR_OK;
}

int pr_hmr_conv_form(pr_hmr_t* h) { return h ? h->conv_form : PR_ERR_INVALID; }

int pr_hmr_plan_counts(pr_hmr_t* h, int B, int* conv_launches, int* winograd_layers) {
  using namespace pr;
  PR_REQUIRE(h && B > 0 && B <= h->max_batch, "pr_hmr_plan_counts: need a handle and a batch within its capacity");
  hmr_plan_counts(*h, B, h->chunk_cap, h->n_chunks, h->profile != 0, conv_launches, winograd_layers);
  return PR_OK;
}

int pr_hmr_profile_enable(pr_hmr_t* h, int on) {
  PR_REQUIRE(h, "pr_hmr_profile_enable: null handle");
  h->profile = on != 0;
  return PR_OK;
}

int pr_hmr_profile_read(pr_hmr_t* h, float* ms, int* launches, double* flops_per_frame, double* mfma_flops_per_frame,
                        int n_layers) {
  using namespace pr;
  PR_REQUIRE(h && n_layers == kNumConv, "pr_hmr_profile_read: need %d layers", kNumConv);
  for (size_t i = 0; i < h->pending.size(); ++i) {
    float t = 0.f;
    PR_HIP(hipEventSynchronize(h->pending[i].second));
    PR_HIP(hipEventElapsedTime(&t, h->pending[i].first, h->pending[i].second));
    h->prof_ms[h->pending_layer[i]] += t;
    h->prof_n[h->pending_layer[i]] += 1;
    (void)hipEventDestroy(h->pending[i].first);
    (void)hipEventDestroy(h->pending[i].second);
  }
  h->pending.clear();
  h->pending_layer.clear();
  for (int i = 0; i < kNumConv; ++i) {
    if (ms) ms[i] = h->prof_ms[i];
    if (launches) launches[i] = h->prof_n[i];
    if (flops_per_frame) flops_per_frame[i] = 0.0;   // a downsample branch fused into its conv3 is counted there
    if (mfma_flops_per_frame) mfma_flops_per_frame[i] = 0.0;
    h->prof_ms[i] = 0.f;
    h->prof_n[i] = 0;
  }
  for (const ConvSpec& c : h->convs) {
    if (flops_per_frame) flops_per_frame[c.layer] = 2.0 * c.macs_per_frame();
    if (mfma_flops_per_frame) {
      mfma_flops_per_frame[c.layer] = 2.0 * c.mfma_macs_per_frame(h->precision == 1 ? 64 : kConvBK);
      // the fused fp32 stem multiplies 13 steps x 12 k per output (stem_pool_f32.hip), not the 192 of the 4x4 x 12 taps
      if (c.out_hw && h->precision == 0 && h->stem_s2d && h->fuse_stem)
        mfma_flops_per_frame[c.layer] = 2.0 * (double)c.Ho() * c.Wo() * c.Cout * 156.0;
    }
  }
  return PR_OK;
}

}  // extern "C"
