// The person detector's handle and device entries (include/poserisk_hip.h, section j8): letterbox, the walk over the 107
// layers (convolutions: det_conv.hip), upsample-into-concat, decode and NMS.  The small kernels index by thread, every loop in
// them has a bound known at launch, and no workgroup waits on another: the candidate list is appended to with one atomic
// add per candidate and ORDERED afterwards by (score, flat index), a total order, so the result does not depend on who
// appended first.
#include <algorithm>
#include <memory>

#include "det_conv.h"
#include "det_host.h"
#include "fence.h"
#include "kernel_vocab.h"

struct pr_det {
  int device = 0, S_h = 0, S_w = 0, max_batch = 0, fence = 0;
  int precision = 0;                       // 0: fp32, 1: the bf16 contract (activations bf16, head tensors fp32)
  pr::DetPlan plan;
  float* packed = nullptr;                 // the folded weights: pr_det_fold_pack's layout, or pr_det_fold_pack_bf16's
  std::vector<int64_t> pack_off_bf16;      // bf16: per layer the byte offset of its bias in `packed`
  std::vector<float*> slots;               // activation buffers, max_batch frames of plan.slot_frame_bytes each
  std::vector<size_t> slot_bytes;
  float* canvas = nullptr;                 // pr_det_detect's letterboxed input, f32[max_batch,S_h,S_w,4]
  float* cand = nullptr;                   // f32[max_batch][cells][6]: score, flat index (as int bits), x1, y1, x2, y2
  int32_t* cand_count = nullptr;           // i32[2][max_batch]: the candidate counts, then the decode kernel's status flags
  int cells = 0;                           // candidates a frame can have: 3 * (sum of the three grids)
  std::vector<void*> allocs;
};

namespace pr {
namespace {

#pragma clang fp contract(off)

constexpr int kDetThreads = 256;
constexpr int kNmsThreads = PR_DET_MAX_CAND;
constexpr int kHeadLayer[3] = {81, 93, 105};
__constant__ float kAnchors[9][2] = {{10, 13}, {16, 30}, {33, 23}, {30, 61}, {62, 45}, {59, 119}, {116, 90}, {156, 198}, {373, 326}};

// ---- letterbox ---------------------------------------------------------------------------------------------------
struct LetterboxParams {
  const uint8_t* src;
  float* dst;
  int B, H, W, S_h, S_w, h2, w2, ox, oy, mode, bgr;
};

// One axis' tap of section j3 for destination sample i: csrc/resize_host.cc's expressions in the same precisions
__device__ __forceinline__ void resize_tap(int S, int d, int i, int* s0, int* c0, int* c1) {
  const double scale = 1.0 / ((double)d / S);
  float f = (float)__dsub_rn(__dmul_rn(i + 0.5, scale), 0.5);
  int s = (int)floorf(f);
  f -= (float)s;
  if (s < 0) s = 0, f = 0.f;
  if (s >= S - 1) s = S - 1, f = 0.f;
  *s0 = s;
  *c0 = (int)rintf((1.f - f) * 2048.f);
  *c1 = (int)rintf(f * 2048.f);
}

__global__ void __launch_bounds__(kDetThreads) det_letterbox_kernel(LetterboxParams p) {
  const long g = (long)blockIdx.x * kDetThreads + threadIdx.x;
  const long total = (long)p.B * p.S_h * p.S_w;
  if (g >= total) return;
  const int x = (int)(g % p.S_w), y = (int)((g / p.S_w) % p.S_h);
  const long b = g / ((long)p.S_w * p.S_h);
  const int ix = x - p.ox, iy = y - p.oy;
  unsigned v[3] = {128u, 128u, 128u};
  if (ix >= 0 && ix < p.w2 && iy >= 0 && iy < p.h2) {
    const uint8_t* s = p.src + b * ((long)p.H * p.W * 3);
    const long pitch = (long)p.W * 3;
    if (p.mode == PR_RESIZE_COPY) {
      for (int c = 0; c < 3; ++c) v[c] = s[iy * pitch + 3 * ix + c];
    } else if (p.mode == PR_RESIZE_HALF) {
      const uint8_t* q = s + (long)(2 * iy) * pitch + 6 * ix;
      for (int c = 0; c < 3; ++c) v[c] = (unsigned)(q[c] + q[3 + c] + q[pitch + c] + q[pitch + 3 + c] + 2) >> 2;
    } else {
      int x0, a0, a1, y0, b0, b1;
      resize_tap(p.W, p.w2, ix, &x0, &a0, &a1);
      resize_tap(p.H, p.h2, iy, &y0, &b0, &b1);
      x0 = min(max(x0, 0), p.W - 1), y0 = min(max(y0, 0), p.H - 1);
      const int x1 = min(x0 + 1, p.W - 1), y1 = min(y0 + 1, p.H - 1);
      const uint8_t* r0 = s + y0 * pitch;
      const uint8_t* r1 = s + y1 * pitch;
      for (int c = 0; c < 3; ++c) {
        const int t0 = r0[3 * x0 + c] * a0 + r0[3 * x1 + c] * a1, t1 = r1[3 * x0 + c] * a0 + r1[3 * x1 + c] * a1;
        v[c] = (unsigned)((((b0 * (t0 >> 4)) >> 16) + ((b1 * (t1 >> 4)) >> 16) + 2) >> 2);
      }
    }
  }
  const float k = 1.f / 255.f;
  const f32x4 o = {(float)v[p.bgr ? 2 : 0] * k, (float)v[1] * k, (float)v[p.bgr ? 0 : 2] * k, 0.f};
  *reinterpret_cast<f32x4*>(p.dst + 4 * g) = o;
}

// h', w', ox, oy of the header's integer rule
void letterbox_geometry(int H, int W, int S_h, int S_w, int* h2, int* w2, int* ox, int* oy) {
  if ((long)W * S_h >= (long)H * S_w) {
    *w2 = S_w;
    *h2 = (int)std::min<long>(S_h, std::max<long>(1, (2l * H * S_w + W) / (2l * W)));
  } else {
    *h2 = S_h;
    *w2 = (int)std::min<long>(S_w, std::max<long>(1, (2l * W * S_h + H) / (2l * H)));
  }
  *ox = (S_w - *w2) / 2, *oy = (S_h - *h2) / 2;
}

int letterbox_launch(const uint8_t* frames, int B, int H, int W, int bgr, int S_h, int S_w, float* x, hipStream_t stream) {
  LetterboxParams p;
  p.src = frames, p.dst = x, p.B = B, p.H = H, p.W = W, p.S_h = S_h, p.S_w = S_w, p.bgr = bgr != 0;
  letterbox_geometry(H, W, S_h, S_w, &p.h2, &p.w2, &p.ox, &p.oy);
  p.mode = (H == p.h2 && W == p.w2) ? PR_RESIZE_COPY : (W == 2 * p.w2 && H == 2 * p.h2) ? PR_RESIZE_HALF : PR_RESIZE_LINEAR;
  const long blocks = ceil_div((long)B * S_h * S_w, (long)kDetThreads);
  hipLaunchKernelGGL(det_letterbox_kernel, dim3((unsigned)blocks), dim3(kDetThreads), 0, stream, p);
  return check_launch("det_letterbox_kernel");
}

// ---- upsample-into-concat ------------------------------------------------------------------------------------------
// out[b][y][x][c] = c < Ca ? a[b][y >> sa][x >> sa][c] : bsrc[b][y][x][c - Ca]; a's grid is (gh >> sa) x (gw >> sa).  Channels
// are multiples of 4: one 16-byte chunk a thread.  sa = 1, Cb = 0: the upsample layer alone; sa = 0: a plain concatenation.
struct ConcatParams {
  const float* a;
  const float* b;
  float* out;
  int B, gh, gw, Ca, Cb, sa;
};
__global__ void __launch_bounds__(kDetThreads) det_concat_kernel(ConcatParams p) {
  const int C4 = (p.Ca + p.Cb) >> 2;
  const long g = (long)blockIdx.x * kDetThreads + threadIdx.x;
  const long total = (long)p.B * p.gh * p.gw * C4;
  if (g >= total) return;
  const int c = 4 * (int)(g % C4);
  const long pix = g / C4;
  const int x = (int)(pix % p.gw), y = (int)((pix / p.gw) % p.gh);
  const long b = pix / ((long)p.gw * p.gh);
  f32x4 v;
  if (c < p.Ca) {
    const int ah = p.gh >> p.sa, aw = p.gw >> p.sa;
    v = *reinterpret_cast<const f32x4*>(p.a + ((b * ah + (y >> p.sa)) * aw + (x >> p.sa)) * p.Ca + c);
  } else {
    v = *reinterpret_cast<const f32x4*>(p.b + pix * p.Cb + (c - p.Ca));
  }
  *reinterpret_cast<f32x4*>(p.out + pix * (p.Ca + p.Cb) + c) = v;
}

int concat_launch(const float* a, const float* b, float* out, int B, int gh, int gw, int Ca, int Cb, int sa, hipStream_t stream) {
  PR_REQUIRE(Ca % 4 == 0 && Cb % 4 == 0 && Ca > 0, "detector: concat of %d + %d 4-byte words a pixel", Ca, Cb);
  ConcatParams p{a, b, out, B, gh, gw, Ca, Cb, sa};
  const long blocks = ceil_div((long)B * gh * gw * ((Ca + Cb) / 4), (long)kDetThreads);
  hipLaunchKernelGGL(det_concat_kernel, dim3((unsigned)blocks), dim3(kDetThreads), 0, stream, p);
  return check_launch("det_concat_kernel");
}

// ---- decode ------------------------------------------------------------------------------------------------------
struct HeadSet {
  const float* t[3];      // f32[B,gh,gw,255] at strides 32, 16, 8
  int gh[3], gw[3];
  int base[3];            // flat index of the head's first cell
  int cells;
};

__device__ __forceinline__ double sigmoid64(double t) { return 1.0 / (1.0 + exp(-t)); }

__device__ __forceinline__ bool finite32(float v) { return fabsf(v) <= 3.402823466e+38f; }      // false for NaN and +-inf

// cand_flag[b] collects PR_DET_STATUS_NONFINITE (zeroed with cand_count; det_nms_kernel folds it into the status): a cell that
// raises it returns before the append, so every appended score and corner is finite.
__global__ void __launch_bounds__(kDetThreads) det_decode_kernel(HeadSet hs, float conf_thres, float* cand, int32_t* cand_count,
                                                                 int32_t* cand_flag) {
  const int flat = blockIdx.x * kDetThreads + threadIdx.x;
  const int b = blockIdx.y;
  if (flat >= hs.cells) return;
  const int hd = flat >= hs.base[2] ? 2 : flat >= hs.base[1] ? 1 : 0;
  const int gh = hs.gh[hd], gw = hs.gw[hd];
  const int r = flat - hs.base[hd];
  const int a = r / (gh * gw), cy = (r / gw) % gh, cx = r % gw;
  const float* t = hs.t[hd] + (((long)b * gh + cy) * gw + cx) * 255 + a * 85;
  if (t[4] != t[4]) {      // a NaN objectness logit: neither above nor below the threshold
    atomicOr(cand_flag + b, PR_DET_STATUS_NONFINITE);
    return;
  }
  const double so = sigmoid64((double)t[4]);
  if (!((float)so >= conf_thres)) return;
  const float c0 = t[5];
  bool person = true;
  for (int c = 1; c < 80; ++c) person = person && !(t[5 + c] > c0);
  if (!person) return;
  const int stride = 32 >> hd, an = 3 * (2 - hd) + a;
  const float bx = (float)((sigmoid64((double)t[0]) + cx) * stride), by = (float)((sigmoid64((double)t[1]) + cy) * stride);
  const float bw = (float)((double)kAnchors[an][0] * exp((double)t[2])), bh = (float)((double)kAnchors[an][1] * exp((double)t[3]));
  const float score = (float)(so * sigmoid64((double)c0));
  const float hw = 0.5f * bw, hh = 0.5f * bh;
  const float x1 = bx - hw, y1 = by - hh, x2 = bx + hw, y2 = by + hh;
  if (!(finite32(score) && finite32(x1) && finite32(y1) && finite32(x2) && finite32(y2))) {
    atomicOr(cand_flag + b, PR_DET_STATUS_NONFINITE);
    return;
  }
  const int slot = atomicAdd(cand_count + b, 1);
  if (slot >= hs.cells) return;      // cannot happen: a cell appends once
  float* o = cand + ((long)b * hs.cells + slot) * 6;
  o[0] = score, o[1] = __int_as_float(flat), o[2] = x1, o[3] = y1, o[4] = x2, o[5] = y2;
}

// ---- order, NMS, output: one workgroup a frame ---------------------------------------------------------------------
__device__ __forceinline__ float det_iou(f32x4 a, f32x4 b) {
  const float iw = fmaxf(fminf(a[2], b[2]) - fmaxf(a[0], b[0]), 0.f), ih = fmaxf(fminf(a[3], b[3]) - fmaxf(a[1], b[1]), 0.f);
  const float inter = iw * ih;
  const float aa = (a[2] - a[0]) * (a[3] - a[1]), ab = (b[2] - b[0]) * (b[3] - b[1]);
  return inter / ((aa + ab) - inter);
}

__global__ void __launch_bounds__(kNmsThreads) det_nms_kernel(const float* cand, const int32_t* cand_count, const int32_t* cand_flag,
                                                              int cells, float nms_thres, int max_det, float* boxes, float* scores,
                                                              int32_t* count, int32_t* status) {
  __shared__ f32x4 sbox[PR_DET_MAX_CAND];
  __shared__ float sscore[PR_DET_MAX_CAND];
  __shared__ int srem[PR_DET_MAX_CAND];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int n = min(max(cand_count[b], 0), cells);
  const float* cb = cand + (long)b * cells * 6;
  // rank = how many candidates come first in (score descending, flat index ascending).  Ranks are distinct: the decode kernel
  // appends no score that is NaN, so of two candidates' scores one is greater or they are equal, and no two candidates share a
  // flat index (a cell appends once): exactly one of two candidates comes before the other, the relation is transitive, and
  // the n ranks are 0..n-1, each once.  Every slot below m = min(n, MAX_CAND) is therefore written exactly once.
  for (int i = tid; i < n; i += kNmsThreads) {
    const float si = cb[6 * i];
    const int fi = __float_as_int(cb[6 * i + 1]);
    int rank = 0;
    for (int j = 0; j < n; ++j) {
      const float sj = cb[6 * j];
      rank += (sj > si || (sj == si && __float_as_int(cb[6 * j + 1]) < fi)) ? 1 : 0;
    }
    if (rank < PR_DET_MAX_CAND) {
      sbox[rank] = f32x4{cb[6 * i + 2], cb[6 * i + 3], cb[6 * i + 4], cb[6 * i + 5]};
      sscore[rank] = si;
    }
  }
  srem[tid] = 0;
  const int m = min(n, PR_DET_MAX_CAND);
  __syncthreads();
  const f32x4 mine = tid < m ? sbox[tid] : f32x4{0.f, 0.f, 0.f, 0.f};
  bool gone = false;
  for (int i = 0; i < m; ++i) {      // m is the same for the whole workgroup: every thread reaches every barrier
    if (tid > i && tid < m && !gone && !srem[i] && det_iou(sbox[i], mine) > nms_thres) gone = true, srem[tid] = 1;
    __syncthreads();
  }
  int pos = 0, kept = 0;
  for (int k = 0; k < m; ++k) {
    const int keep = srem[k] ? 0 : 1;
    pos += (k < tid) ? keep : 0;
    kept += keep;
  }
  const int nout = min(kept, max_det);
  float* ob = boxes + (long)b * max_det * 4;
  float* os = scores + (long)b * max_det;
  if (tid < m && !gone && pos < max_det) {
    ob[4 * pos] = mine[0], ob[4 * pos + 1] = mine[1], ob[4 * pos + 2] = mine[2], ob[4 * pos + 3] = mine[3];
    os[pos] = sscore[tid];
  }
  if (tid >= nout && tid < max_det) {
    ob[4 * tid] = 0.f, ob[4 * tid + 1] = 0.f, ob[4 * tid + 2] = 0.f, ob[4 * tid + 3] = 0.f;
    os[tid] = 0.f;
  }
  if (tid == 0) {
    count[b] = nout;
    status[b] = (n > PR_DET_MAX_CAND ? PR_DET_STATUS_CAND_OVERFLOW : 0) | (kept > max_det ? PR_DET_STATUS_DET_OVERFLOW : 0) |
                (cand_flag[b] & PR_DET_STATUS_NONFINITE);
  }
}

// letterbox pixels -> frame pixels, clipped to the frame
__global__ void __launch_bounds__(kDetThreads) det_unmap_kernel(float* boxes, const int32_t* count, long n_boxes, int max_det, float ox,
                                                                float oy, float sx, float sy, float W, float H) {
  const long g = (long)blockIdx.x * kDetThreads + threadIdx.x;
  if (g >= n_boxes) return;
  if ((int)(g % max_det) >= count[g / max_det]) return;      // a row beyond count stays as it is (pr_det_detect: zero)
  float* q = boxes + 4 * g;
  q[0] = fminf(fmaxf((q[0] - ox) * sx, 0.f), W), q[2] = fminf(fmaxf((q[2] - ox) * sx, 0.f), W);
  q[1] = fminf(fmaxf((q[1] - oy) * sy, 0.f), H), q[3] = fminf(fmaxf((q[3] - oy) * sy, 0.f), H);
}

// pr_det_detect's last step and pr_det_unmap: B * max_det <= 4096 * 1024 boxes, a thread each
int unmap_launch(float* boxes, const int32_t* count, int B, int max_det, int H, int W, int S_h, int S_w, hipStream_t stream) {
  int h2, w2, ox, oy;
  letterbox_geometry(H, W, S_h, S_w, &h2, &w2, &ox, &oy);
  const long n_boxes = (long)B * max_det;
  hipLaunchKernelGGL(det_unmap_kernel, dim3((unsigned)ceil_div(n_boxes, (long)kDetThreads)), dim3(kDetThreads), 0, stream, boxes, count,
                     n_boxes, max_det, (float)ox, (float)oy, (float)W / (float)w2, (float)H / (float)h2, (float)W, (float)H);
  return check_launch("det_unmap_kernel");
}

// ---- the handle ----------------------------------------------------------------------------------------------------
// A tensor of `bytes` in buffer `slot`: on its first byte, or -- internal fence, tail mode -- ending within 15 bytes of its
// last (the offset is kept a multiple of 16 for the 16-byte accesses; a 255-channel head tensor need not be one).
float* placed(const pr_det* h, int slot, size_t bytes) {
  char* base = reinterpret_cast<char*>(h->slots[slot]);
  if (h->fence != 2 || bytes > h->slot_bytes[slot]) return reinterpret_cast<float*>(base);
  return reinterpret_cast<float*>(base + (h->slot_bytes[slot] - bytes) / 16 * 16);
}
size_t tensor_bytes(const pr_det* h, int layer, int B) {
  const auto& P = h->plan;
  return (size_t)B * P.gh[layer] * P.gw[layer] * P.layers[layer].cout * P.elem_bytes[layer];
}
float* tensor_of(const pr_det* h, int layer, int B) {
  const auto& P = h->plan;
  return placed(h, P.slot[layer], tensor_bytes(h, layer, B));
}

template <typename T>
int det_alloc(pr_det* h, T** out, size_t bytes, size_t frame_bytes, const char* name) {
  void* d = nullptr;
  PR_TRY(device_alloc(&d, std::max<size_t>(bytes, 16), h->fence, frame_bytes, "det %s", name));
  h->allocs.push_back(d);
  *out = reinterpret_cast<T*>(d);
  return PR_OK;
}

int det_build(pr_det* h, const float* weights_host, size_t n_floats, double bn_eps) {
  PR_TRY(det_plan(h->S_h, h->S_w, &h->plan, h->precision));
  const auto& P = h->plan;
  const size_t lim = 0x7fffffffu;
  for (int l = 0; l < kDetLayers; ++l)
    PR_REQUIRE((size_t)h->max_batch * P.gh[l] * P.gw[l] * std::max(P.layers[l].cout, 4) * sizeof(float) <= lim &&
                   (size_t)h->max_batch * h->S_h * h->S_w * 4 * sizeof(float) <= lim,
               "pr_det_create: %d frames of %d x %d make an activation tensor of 2 GiB or more; lower max_batch", h->max_batch, h->S_w,
               h->S_h);
  const size_t packed_bytes = h->precision ? pr_det_packed_bytes_bf16(kDetLayers) : pr_det_packed_floats(kDetLayers) * sizeof(float);
  std::vector<float> packed(packed_bytes / sizeof(float));      // both layouts are whole floats long
  if (h->precision) {
    PR_TRY(pr_det_fold_pack_bf16(kDetLayers, weights_host, n_floats, bn_eps, packed.data(), packed_bytes));
    det_pack_offsets_bf16(kDetLayers, &h->pack_off_bf16);
  } else {
    PR_TRY(pr_det_fold_pack(kDetLayers, weights_host, n_floats, bn_eps, packed.data(), packed.size()));
  }
  PR_TRY(det_alloc(h, &h->packed, packed_bytes, 0, "packed weights"));
  PR_HIP(hipMemcpy(h->packed, packed.data(), packed_bytes, hipMemcpyHostToDevice));
  h->slots.resize(P.slot_frame_bytes.size());
  h->slot_bytes.resize(P.slot_frame_bytes.size());
  for (size_t s = 0; s < P.slot_frame_bytes.size(); ++s) {
    char name[32];
    snprintf(name, sizeof name, "act[%zu]", s);
    h->slot_bytes[s] = (P.slot_frame_bytes[s] * h->max_batch + 255) / 256 * 256;
    PR_TRY(det_alloc(h, &h->slots[s], h->slot_bytes[s], P.slot_frame_bytes[s], name));
  }
  h->cells = 0;
  for (int i = 0; i < 3; ++i) h->cells += 3 * P.gh[kHeadLayer[i]] * P.gw[kHeadLayer[i]];
  PR_TRY(det_alloc(h, &h->canvas, (size_t)h->max_batch * h->S_h * h->S_w * 4 * sizeof(float), (size_t)h->S_h * h->S_w * 4 * sizeof(float),
                   "canvas"));
  PR_TRY(det_alloc(h, &h->cand, (size_t)h->max_batch * h->cells * 6 * sizeof(float), (size_t)h->cells * 6 * sizeof(float), "candidates"));
  PR_TRY(det_alloc(h, &h->cand_count, (size_t)2 * h->max_batch * sizeof(int32_t), 0, "candidate counts"));
  PR_HIP(hipDeviceSynchronize());
  return PR_OK;
}

// Layers 0..until on x f32[B,S_h,S_w,4].  heads: where the three head convolutions write (nullptr: the handle's own buffers).
int det_walk(pr_det* h, const float* x, int B, int until, float* const* heads, hipStream_t stream) {
  const auto& P = h->plan;
  const auto& L = P.layers;
  for (int l = 0; l <= until; ++l) {
    const pr_det_layer& c = L[l];
    if (c.type == PR_DET_CONV) {
      const bool fused = l + 1 <= until && L[l + 1].type == PR_DET_SHORTCUT;
      if (h->precision && l > 0) {      // bf16 operands; layer 0 stays on the fp32 kernel below and only stores bf16
        DetConvBf16Problem q;
        q.x = tensor_of(h, l - 1, B);
        q.B = B, q.H = P.gh[l - 1], q.W = P.gw[l - 1];
        q.Cin = c.cin_pad, q.Ho = P.gh[l], q.Wo = P.gw[l], q.Cout = c.cout, q.cout_pad = c.cout_pad, q.kpad = c.kpad;
        q.ksize = c.ksize, q.stride = c.stride, q.leaky = c.bn, q.out_f32 = P.elem_bytes[l] == 4;
        const char* blob = reinterpret_cast<const char*>(h->packed) + h->pack_off_bf16[l];
        q.bias = reinterpret_cast<const float*>(blob);
        q.w = blob + (size_t)c.cout_pad * 4;
        q.res = fused ? tensor_of(h, L[l + 1].from0, B) : nullptr;
        q.y = tensor_of(h, l, B);
        if (heads)
          for (int i = 0; i < 3; ++i)
            if (l == kHeadLayer[i]) q.y = heads[i];
        PR_TRY(det_conv_bf16_launch(q, stream));
        if (fused) ++l;
        continue;
      }
      DetConvProblem p;
      p.x = l == 0 ? x : tensor_of(h, l - 1, B);
      p.B = B, p.H = l == 0 ? h->S_h : P.gh[l - 1], p.W = l == 0 ? h->S_w : P.gw[l - 1];
      p.Cin = c.cin_pad, p.Ho = P.gh[l], p.Wo = P.gw[l], p.Cout = c.cout, p.cout_pad = c.cout_pad, p.kpad = c.kpad;
      p.ksize = c.ksize, p.stride = c.stride, p.leaky = c.bn, p.out_bf16 = h->precision;
      p.bias = h->packed + c.pack_offset;      // layer 0 begins both blobs and has the same layout in both
      p.w = p.bias + c.cout_pad;
      p.res = fused ? tensor_of(h, L[l + 1].from0, B) : nullptr;
      p.y = tensor_of(h, l, B);
      if (heads)
        for (int i = 0; i < 3; ++i)
          if (l == kHeadLayer[i]) p.y = heads[i];
      PR_TRY(det_conv_launch(p, stream));
      if (fused) ++l;
    } else if (c.type == PR_DET_UPSAMPLE) {
      // the copy kernel moves 16-byte chunks of 4-byte words: two bf16 channels make one word (channels are multiples of 8)
      const int cw = h->precision ? 2 : 1;
      // with the concatenation behind it wanted too, the upsampled tensor is never written: one kernel fills the route's
      const bool into = l + 1 <= until && L[l + 1].type == PR_DET_ROUTE && L[l + 1].from0 == l && L[l + 1].from1 >= 0;
      if (into) {
        const int o = l + 1;
        PR_TRY(concat_launch(tensor_of(h, l - 1, B), tensor_of(h, L[o].from1, B), tensor_of(h, o, B), B, P.gh[o], P.gw[o], c.cout / cw,
                             L[L[o].from1].cout / cw, 1, stream));
        ++l;
      } else {
        PR_TRY(concat_launch(tensor_of(h, l - 1, B), nullptr, tensor_of(h, l, B), B, P.gh[l], P.gw[l], c.cout / cw, 0, 1, stream));
      }
    } else if (c.type == PR_DET_ROUTE && c.from1 >= 0) {
      const int cw = h->precision ? 2 : 1;
      PR_TRY(concat_launch(tensor_of(h, c.from0, B), tensor_of(h, c.from1, B), tensor_of(h, l, B), B, P.gh[l], P.gw[l],
                           L[c.from0].cout / cw, L[c.from1].cout / cw, 0, stream));
    } else {
      PR_REQUIRE(c.type != PR_DET_SHORTCUT, "detector: internal error, the shortcut at layer %d has no convolution in front", l);
    }
  }
  return PR_OK;
}

int det_post(pr_det* h, const float* const* heads, int B, float conf_thres, float nms_thres, int max_det, float* boxes, float* scores,
             int32_t* count, int32_t* status, hipStream_t stream) {
  const auto& P = h->plan;
  HeadSet hs;
  hs.cells = 0;
  for (int i = 0; i < 3; ++i) {
    hs.t[i] = heads[i], hs.gh[i] = P.gh[kHeadLayer[i]], hs.gw[i] = P.gw[kHeadLayer[i]];
    hs.base[i] = hs.cells;
    hs.cells += 3 * hs.gh[i] * hs.gw[i];
  }
  int32_t* cand_flag = h->cand_count + h->max_batch;
  PR_HIP(hipMemsetAsync(h->cand_count, 0, (size_t)2 * h->max_batch * sizeof(int32_t), stream));
  hipLaunchKernelGGL(det_decode_kernel, dim3((unsigned)ceil_div(hs.cells, kDetThreads), (unsigned)B), dim3(kDetThreads), 0, stream, hs,
                     conf_thres, h->cand, h->cand_count, cand_flag);
  PR_TRY(check_launch("det_decode_kernel"));
  hipLaunchKernelGGL(det_nms_kernel, dim3((unsigned)B), dim3(kNmsThreads), 0, stream, (const float*)h->cand,
                     (const int32_t*)h->cand_count, (const int32_t*)cand_flag, hs.cells, nms_thres, max_det, boxes, scores, count, status);
  return check_launch("det_nms_kernel");
}

int check_common(const pr_det* h, int B, const char* what) {
  PR_REQUIRE(h, "%s: null handle", what);
  PR_REQUIRE(B >= 0, "%s: B = %d", what, B);
  if (B > h->max_batch) {
    set_error("%s: B = %d, but the handle was created for max_batch = %d", what, B, h->max_batch);
    return PR_ERR_CAPACITY;
  }
  return PR_OK;
}
int check_post_args(float conf_thres, float nms_thres, int max_det, const void* boxes, const void* scores, const void* count,
                    const void* status, const char* what) {
  PR_REQUIRE(conf_thres >= 0.f && conf_thres <= 1.f, "%s: conf_thres = %g, must lie in [0, 1]", what, conf_thres);
  PR_REQUIRE(nms_thres >= 0.f && nms_thres <= 1.f, "%s: nms_thres = %g, must lie in [0, 1]", what, nms_thres);
  PR_REQUIRE(max_det >= 1 && max_det <= PR_DET_MAX_CAND, "%s: max_det = %d, must lie in 1..%d", what, max_det, PR_DET_MAX_CAND);
  PR_REQUIRE(boxes, "%s: null boxes_dev", what);
  PR_REQUIRE(scores, "%s: null scores_dev", what);
  PR_REQUIRE(count, "%s: null count_dev", what);
  PR_REQUIRE(status, "%s: null status_dev", what);
  return PR_OK;
}
int check_frames(const void* frames, int H, int W, const char* what) {
  PR_REQUIRE(frames, "%s: null frames_dev", what);
  PR_REQUIRE(H >= 1 && H <= PR_RESIZE_MAX_SIDE && W >= 1 && W <= PR_RESIZE_MAX_SIDE, "%s: frames of %d x %d: every side must lie in 1..%d",
             what, W, H, PR_RESIZE_MAX_SIDE);
  return PR_OK;
}

}  // namespace
}  // namespace pr

extern "C" {

int pr_det_create(int device, const float* weights_host, size_t n_floats, int S_h, int S_w, int max_batch, double bn_eps, pr_det_t** out) {
  return pr_det_create_p(device, weights_host, n_floats, S_h, S_w, max_batch, bn_eps, 0, out);
}

// the messages keep pr_det_create's name: it is the fp32 entry's text, and the bf16 handle is refused for the same reasons
int pr_det_create_p(int device, const float* weights_host, size_t n_floats, int S_h, int S_w, int max_batch, double bn_eps, int precision,
                    pr_det_t** out) {
  using namespace pr;
  PR_REQUIRE(out, "pr_det_create: null out");
  PR_REQUIRE(precision == 0 || precision == 1, "pr_det_create_p: precision = %d, must be 0 (fp32) or 1 (bf16)", precision);
  PR_REQUIRE(weights_host, "pr_det_create: null weights_host");
  PR_REQUIRE(n_floats == pr_det_weight_floats(kDetLayers), "pr_det_create: n_floats = %zu, but the network holds %zu", n_floats,
             pr_det_weight_floats(kDetLayers));
  PR_REQUIRE(S_h >= 32 && S_w >= 32 && S_h % 32 == 0 && S_w % 32 == 0 && S_h <= 4096 && S_w <= 4096,
             "pr_det_create: the network input %d x %d (S_w x S_h) must be multiples of 32 in 32..4096", S_w, S_h);
  PR_REQUIRE(max_batch >= 1 && max_batch <= 4096, "pr_det_create: max_batch = %d, must lie in 1..4096", max_batch);
  PR_REQUIRE(bn_eps > 0 && bn_eps < 1, "pr_det_create: bn_eps = %g, must lie in (0, 1)", bn_eps);
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
    set_error("pr_det_create: no HIP device visible");
    return PR_ERR_NO_DEVICE;
  }
  PR_REQUIRE(device >= 0 && device < ndev, "pr_det_create: device %d of %d", device, ndev);
  DeviceGuard g(device);
  PR_TRY(refuse_under_declared_capture("pr_det_create"));
  std::unique_ptr<pr_det> h(new pr_det);
  h->device = device, h->S_h = S_h, h->S_w = S_w, h->max_batch = max_batch, h->precision = precision;
  h->fence = fence_mode_from_env();
  const int st = det_build(h.get(), weights_host, n_floats, bn_eps);
  if (st != PR_OK) {
    for (void* p : h->allocs) device_free(p);
    return st;
  }
  *out = h.release();
  return PR_OK;
}

int pr_det_destroy(pr_det_t* h) {
  if (!h) return PR_OK;
  pr::DeviceGuard g(h->device);
  PR_TRY(pr::refuse_under_declared_capture("pr_det_destroy"));   // the handle stays valid: destroy it after the capture
  for (void* p : h->allocs) pr::device_free(p);
  delete h;
  return PR_OK;
}

int pr_det_input_size(const pr_det_t* h, int* S_h, int* S_w) {
  using namespace pr;
  PR_REQUIRE(h && S_h && S_w, "pr_det_input_size: null argument");
  *S_h = h->S_h, *S_w = h->S_w;
  return PR_OK;
}

int pr_det_max_batch(const pr_det_t* h) { return h ? h->max_batch : 0; }

int pr_det_precision(const pr_det_t* h) { return h ? h->precision : -1; }

int pr_det_elem_bytes(const pr_det_t* h, int layer) {
  return h && layer >= 0 && layer < pr::kDetLayers ? h->plan.elem_bytes[layer] : 0;
}

int pr_det_grid(const pr_det_t* h, int layer, int* gh, int* gw, int* channels) {
  using namespace pr;
  PR_REQUIRE(h && gh && gw && channels, "pr_det_grid: null argument");
  PR_REQUIRE(layer >= 0 && layer < kDetLayers, "pr_det_grid: layer = %d, must lie in 0..%d", layer, kDetLayers - 1);
  *gh = h->plan.gh[layer], *gw = h->plan.gw[layer], *channels = h->plan.layers[layer].cout;
  return PR_OK;
}

int pr_det_conv_nhwc(const float* x_dev, const float* packed_dev, const float* res_dev, float* y_dev, int B, int H, int W, int Cin, int Cout,
                     int ksize, int stride, int leaky, void* stream) {
  using namespace pr;
  PR_REQUIRE(x_dev, "pr_det_conv_nhwc: null x_dev");
  PR_REQUIRE(packed_dev, "pr_det_conv_nhwc: null packed_dev");
  PR_REQUIRE(y_dev, "pr_det_conv_nhwc: null y_dev");
  PR_REQUIRE(B >= 0 && Cout >= 1 && Cout <= 65536 && Cin >= 4 && Cin <= 65536, "pr_det_conv_nhwc: B %d, Cin %d, Cout %d", B, Cin, Cout);
  PR_REQUIRE(ksize == 1 || ksize == 3, "pr_det_conv_nhwc: ksize = %d, must be 1 or 3", ksize);
  PR_REQUIRE(stride == 1 || stride == 2, "pr_det_conv_nhwc: stride = %d, must be 1 or 2", stride);
  PR_REQUIRE(H >= 1 && W >= 1 && H <= 65536 && W <= 65536, "pr_det_conv_nhwc: H %d, W %d", H, W);
  if (B == 0) return PR_OK;
  DetConvProblem p;
  p.x = x_dev, p.res = res_dev, p.y = y_dev, p.B = B, p.H = H, p.W = W, p.Cin = Cin, p.Cout = Cout, p.ksize = ksize, p.stride = stride;
  p.leaky = leaky != 0;
  p.Ho = (H + 2 * (ksize / 2) - ksize) / stride + 1, p.Wo = (W + 2 * (ksize / 2) - ksize) / stride + 1;
  p.cout_pad = (Cout + kDetCoutTile - 1) / kDetCoutTile * kDetCoutTile;
  p.kpad = (ksize * ksize * Cin + kDetKTile - 1) / kDetKTile * kDetKTile;
  p.bias = packed_dev, p.w = packed_dev + p.cout_pad;
  return det_conv_launch(p, (hipStream_t)stream);
}

int pr_det_conv_nhwc_bf16(const void* x_dev, const void* packed_dev, const void* res_dev, void* y_dev, int B, int H, int W, int Cin, int Cout,
                          int ksize, int stride, int leaky, int out_f32, void* stream) {
  using namespace pr;
  PR_REQUIRE(x_dev, "pr_det_conv_nhwc_bf16: null x_dev");
  PR_REQUIRE(packed_dev, "pr_det_conv_nhwc_bf16: null packed_dev");
  PR_REQUIRE(y_dev, "pr_det_conv_nhwc_bf16: null y_dev");
  PR_REQUIRE(B >= 0 && Cout >= 1 && Cout <= 65536, "pr_det_conv_nhwc_bf16: B %d, Cout %d", B, Cout);
  PR_REQUIRE(Cin >= 8 && Cin <= 65536 && Cin % 8 == 0, "pr_det_conv_nhwc_bf16: Cin = %d, must be a multiple of 8 in 8..65536", Cin);
  PR_REQUIRE(ksize == 1 || ksize == 3, "pr_det_conv_nhwc_bf16: ksize = %d, must be 1 or 3", ksize);
  PR_REQUIRE(stride == 1 || stride == 2, "pr_det_conv_nhwc_bf16: stride = %d, must be 1 or 2", stride);
  PR_REQUIRE(H >= 1 && W >= 1 && H <= 65536 && W <= 65536, "pr_det_conv_nhwc_bf16: H %d, W %d", H, W);
  if (B == 0) return PR_OK;
  DetConvBf16Problem p;
  p.x = x_dev, p.res = res_dev, p.y = y_dev, p.B = B, p.H = H, p.W = W, p.Cin = Cin, p.Cout = Cout, p.ksize = ksize, p.stride = stride;
  p.leaky = leaky != 0, p.out_f32 = out_f32 != 0;
  p.Ho = (H + 2 * (ksize / 2) - ksize) / stride + 1, p.Wo = (W + 2 * (ksize / 2) - ksize) / stride + 1;
  p.cout_pad = (Cout + kDetCoutTile - 1) / kDetCoutTile * kDetCoutTile;
  p.kpad = (ksize * ksize * Cin + kDetKTile - 1) / kDetKTile * kDetKTile;
  p.bias = static_cast<const float*>(packed_dev), p.w = static_cast<const char*>(packed_dev) + (size_t)p.cout_pad * 4;
  return det_conv_bf16_launch(p, (hipStream_t)stream);
}

int pr_det_letterbox(pr_det_t* h, const uint8_t* frames_dev, int B, int H, int W, int bgr, float* x_dev, void* stream) {
  using namespace pr;
  PR_TRY(check_common(h, B, "pr_det_letterbox"));
  PR_TRY(check_frames(frames_dev, H, W, "pr_det_letterbox"));
  PR_REQUIRE(x_dev, "pr_det_letterbox: null x_dev");
  if (B == 0) return PR_OK;
  return letterbox_launch(frames_dev, B, H, W, bgr, h->S_h, h->S_w, x_dev, (hipStream_t)stream);
}

int pr_det_network(pr_det_t* h, const float* x_dev, int B, float* head32_dev, float* head16_dev, float* head8_dev, void* stream) {
  using namespace pr;
  PR_TRY(check_common(h, B, "pr_det_network"));
  PR_REQUIRE(x_dev, "pr_det_network: null x_dev");
  PR_REQUIRE(head32_dev, "pr_det_network: null head32_dev");
  PR_REQUIRE(head16_dev, "pr_det_network: null head16_dev");
  PR_REQUIRE(head8_dev, "pr_det_network: null head8_dev");
  if (B == 0) return PR_OK;
  float* const heads[3] = {head32_dev, head16_dev, head8_dev};
  return det_walk(h, x_dev, B, kDetLayers - 1, heads, (hipStream_t)stream);
}

int pr_det_network_until(pr_det_t* h, const float* x_dev, int B, int layer, void* act_dev, void* stream) {
  using namespace pr;
  PR_TRY(check_common(h, B, "pr_det_network_until"));
  PR_REQUIRE(x_dev, "pr_det_network_until: null x_dev");
  PR_REQUIRE(act_dev, "pr_det_network_until: null act_dev");
  PR_REQUIRE(layer >= 0 && layer < kDetLayers, "pr_det_network_until: layer = %d, must lie in 0..%d", layer, kDetLayers - 1);
  if (B == 0) return PR_OK;
  PR_TRY(det_walk(h, x_dev, B, layer, nullptr, (hipStream_t)stream));
  PR_HIP(hipMemcpyAsync(act_dev, tensor_of(h, layer, B), tensor_bytes(h, layer, B), hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return PR_OK;
}

int pr_det_postprocess(pr_det_t* h, const float* head32_dev, const float* head16_dev, const float* head8_dev, int B, float conf_thres,
                       float nms_thres, int max_det, float* boxes_dev, float* scores_dev, int32_t* count_dev, int32_t* status_dev,
                       void* stream) {
  using namespace pr;
  PR_TRY(check_common(h, B, "pr_det_postprocess"));
  PR_REQUIRE(head32_dev, "pr_det_postprocess: null head32_dev");
  PR_REQUIRE(head16_dev, "pr_det_postprocess: null head16_dev");
  PR_REQUIRE(head8_dev, "pr_det_postprocess: null head8_dev");
  PR_TRY(check_post_args(conf_thres, nms_thres, max_det, boxes_dev, scores_dev, count_dev, status_dev, "pr_det_postprocess"));
  if (B == 0) return PR_OK;
  const float* const heads[3] = {head32_dev, head16_dev, head8_dev};
  return det_post(h, heads, B, conf_thres, nms_thres, max_det, boxes_dev, scores_dev, count_dev, status_dev, (hipStream_t)stream);
}

int pr_det_detect(pr_det_t* h, const uint8_t* frames_dev, int B, int H, int W, int bgr, float conf_thres, float nms_thres, int max_det,
                  float* boxes_dev, float* scores_dev, int32_t* count_dev, int32_t* status_dev, void* stream) {
  using namespace pr;
  PR_TRY(check_common(h, B, "pr_det_detect"));
  PR_TRY(check_frames(frames_dev, H, W, "pr_det_detect"));
  PR_TRY(check_post_args(conf_thres, nms_thres, max_det, boxes_dev, scores_dev, count_dev, status_dev, "pr_det_detect"));
  if (B == 0) return PR_OK;
  hipStream_t s = (hipStream_t)stream;
  PR_TRY(letterbox_launch(frames_dev, B, H, W, bgr, h->S_h, h->S_w, h->canvas, s));
  PR_TRY(det_walk(h, h->canvas, B, kDetLayers - 1, nullptr, s));
  const float* const heads[3] = {tensor_of(h, kHeadLayer[0], B), tensor_of(h, kHeadLayer[1], B), tensor_of(h, kHeadLayer[2], B)};
  PR_TRY(det_post(h, heads, B, conf_thres, nms_thres, max_det, boxes_dev, scores_dev, count_dev, status_dev, s));
  return unmap_launch(boxes_dev, count_dev, B, max_det, H, W, h->S_h, h->S_w, s);
}

int pr_det_unmap(float* boxes_dev, const int32_t* count_dev, int B, int max_det, int H, int W, int S_h, int S_w, void* stream) {
  using namespace pr;
  PR_REQUIRE(boxes_dev, "pr_det_unmap: null boxes_dev");
  PR_REQUIRE(count_dev, "pr_det_unmap: null count_dev");
  PR_REQUIRE(B >= 0 && B <= 4096, "pr_det_unmap: B = %d, must lie in 0..4096", B);
  PR_REQUIRE(max_det >= 1 && max_det <= PR_DET_MAX_CAND, "pr_det_unmap: max_det = %d, must lie in 1..%d", max_det, PR_DET_MAX_CAND);
  PR_TRY(check_frames(boxes_dev, H, W, "pr_det_unmap"));
  PR_REQUIRE(S_h >= 32 && S_w >= 32 && S_h % 32 == 0 && S_w % 32 == 0 && S_h <= 4096 && S_w <= 4096,
             "pr_det_unmap: the network input %d x %d (S_w x S_h) must be multiples of 32 in 32..4096", S_w, S_h);
  if (B == 0) return PR_OK;
  return unmap_launch(boxes_dev, count_dev, B, max_det, H, W, S_h, S_w, (hipStream_t)stream);
}

}  // extern "C"
