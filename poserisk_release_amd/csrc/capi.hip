// C-ABI entry points that are thin wrappers (error state, stand-alone kernels, the per-batch
// driver).  pr_hmr_* lives in hmr.hip, pr_smpl_* in smpl.hip.
// The nine stand-alone test entries (pr_conv2d_nhwc .. pr_stem_pool_f32_nhwc) are argument checks, a weight layout from
// host_plan.cc's packers -- the ones the encoder's plan uploads -- and a launch, inside one frame: StandAlone.
#include <optional>
#include <vector>

#include "conv_igemm.h"
#include "fence.h"
#include "frame_kernels.h"

namespace pr {
namespace {
thread_local std::string g_last_error;
thread_local bool g_stream_declared = false;
thread_local hipStream_t g_declared_stream = nullptr;
}
void declared_stream(bool* declared, hipStream_t* s) {
  *declared = g_stream_declared;
  *s = g_declared_stream;
}
void set_error(const char* fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_last_error = buf;
}
}  // namespace pr

#define PR_STR_(x) #x
#define PR_STR(x) PR_STR_(x)

extern "C" {

const char* pr_last_error(void) { return pr::g_last_error.c_str(); }
int pr_abi_version(void) { return 16; }

int pr_declare_stream(void* stream, int declared) {
  pr::g_stream_declared = declared != 0;
  pr::g_declared_stream = declared ? (hipStream_t)stream : nullptr;
  return PR_OK;
}

// What this binary is: the shipped build says "release"; ablation / experiment builds (POSERISK_CXXFLAGS) name their macros,
// so that a bench record taken on one cannot be mistaken for the shipped library's.
const char* pr_build_info(void) {
  return "gfx950"
#ifdef PR_TIMING_HOOKS
         " +PR_TIMING_HOOKS(results may be wrong)"
#endif
#ifdef PR_EXPERIMENT
         " +PR_EXPERIMENT=" PR_STR(PR_EXPERIMENT)
#endif
#ifdef PR_JPEG_SYNC_SUBSEQ_BYTES
         " +PR_JPEG_SYNC_SUBSEQ_BYTES=" PR_STR(PR_JPEG_SYNC_SUBSEQ_BYTES)
#endif
#ifdef PR_JPEG_SYNC_MAX_ROUNDS
         " +PR_JPEG_SYNC_MAX_ROUNDS=" PR_STR(PR_JPEG_SYNC_MAX_ROUNDS)
#endif
#ifdef PR_JPEG_SYNC_WAVES_PER_CU
         " +PR_JPEG_SYNC_WAVES_PER_CU=" PR_STR(PR_JPEG_SYNC_WAVES_PER_CU)
#endif
#if !defined(PR_TIMING_HOOKS) && !defined(PR_EXPERIMENT) && !defined(PR_JPEG_SYNC_SUBSEQ_BYTES) && \
    !defined(PR_JPEG_SYNC_MAX_ROUNDS) && !defined(PR_JPEG_SYNC_WAVES_PER_CU)
         " release"
#endif
      ;
}

int pr_rot6d_to_rotmat(const float* pose6d_dev, int N, float* rotmat_dev, void* stream) {
  PR_REQUIRE(pose6d_dev && rotmat_dev && N >= 0, "pr_rot6d_to_rotmat: bad argument");
  return pr::launch_rot6d(pose6d_dev, rotmat_dev, (long)N * 24, (hipStream_t)stream);
}

int pr_pose_to_euler(const float* rotmat_dev, int N, float* axis_angle_dev, double* euler_deg_dev,
                     int32_t* status_dev, void* stream) {
  PR_REQUIRE(rotmat_dev && axis_angle_dev && euler_deg_dev && N >= 0, "pr_pose_to_euler: bad argument");
  return pr::launch_pose_to_euler(rotmat_dev, N, axis_angle_dev, euler_deg_dev, status_dev,
                                  (hipStream_t)stream);
}

int pr_axis_angle_to_euler(const float* axis_angle_dev, int N, double* euler_deg_dev, int32_t* status_dev,
                           void* stream) {
  PR_REQUIRE(axis_angle_dev && euler_deg_dev && N >= 0, "pr_axis_angle_to_euler: bad argument");
  return pr::launch_pose_to_euler(nullptr, N, const_cast<float*>(axis_angle_dev), euler_deg_dev, status_dev,
                                  (hipStream_t)stream);
}

int pr_reba(const double* euler_deg_dev, int N, const pr_reba_info* info, int32_t* out_dev, void* stream) {
  PR_REQUIRE(euler_deg_dev && info && out_dev && N >= 0, "pr_reba: bad argument");
  return pr::launch_reba(euler_deg_dev, N, *info, out_dev, (hipStream_t)stream);
}

int pr_rula(const double* euler_deg_dev, int N, const pr_rula_info* info, int32_t* out_dev, void* stream) {
  PR_REQUIRE(euler_deg_dev && info && out_dev && N >= 0, "pr_rula: bad argument");
  return pr::launch_rula(euler_deg_dev, N, *info, out_dev, (hipStream_t)stream);
}

int pr_reba_rows(const double* euler_deg_dev, int N, const pr_reba_info* info, const int32_t* activity_rows_dev, int32_t* out_dev,
                 void* stream) {
  PR_REQUIRE(euler_deg_dev && info && out_dev && N >= 0, "pr_reba_rows: bad argument");
  PR_REQUIRE((const void*)activity_rows_dev != (const void*)out_dev, "pr_reba_rows: activity_rows is the output");
  return pr::launch_reba(euler_deg_dev, N, *info, out_dev, (hipStream_t)stream, activity_rows_dev);
}

int pr_rula_rows(const double* euler_deg_dev, int N, const pr_rula_info* info, const int32_t* muscle_rows_dev, int32_t* out_dev,
                 void* stream) {
  PR_REQUIRE(euler_deg_dev && info && out_dev && N >= 0, "pr_rula_rows: bad argument");
  PR_REQUIRE((const void*)muscle_rows_dev != (const void*)out_dev, "pr_rula_rows: muscle_rows is the output");
  return pr::launch_rula(euler_deg_dev, N, *info, out_dev, (hipStream_t)stream, muscle_rows_dev);
}

int pr_crop_frames(const uint8_t* frames_dev, int F, int H, int W, int bgr, const int32_t* frame_idx_dev,
                   const float* bboxes_dev, int N, float scale, float* crops_dev, int32_t* status_dev,
                   void* stream) {
  PR_REQUIRE(frames_dev && bboxes_dev && crops_dev, "pr_crop_frames: null argument");
  PR_REQUIRE(F > 0 && H > 0 && W > 0 && H < 32768 && W < 32768 && N >= 0 && scale > 0, "pr_crop_frames: bad geometry");
  PR_REQUIRE(frame_idx_dev || N <= F, "pr_crop_frames: %d boxes for %d frames without a frame index", N, F);
  return pr::launch_crop_frames(frames_dev, F, H, W, bgr, frame_idx_dev, bboxes_dev, N, scale, crops_dev,
                                status_dev, (hipStream_t)stream);
}

int pr_conv_num_tile_cfgs(void) { return pr::conv_num_tile_cfgs(); }

}  // extern "C"

namespace pr {
namespace {

// The frame of every stand-alone test entry: the caller's device, no allocation inside a capture, the call's device buffers
// and the timing events freed on every return path, the launch (and, for `repeats`, the event-timed loop) followed by the
// synchronisation the buffers must outlive.  A failed upload / device_alloc yields null and is what run() then returns
// instead of launching.
class StandAlone {
 public:
  hipStream_t s = nullptr;
  ~StandAlone() {
    for (void* p : bufs_) device_free(p);      // (internal fence: a damaged guard is kept for the next pr_fence_check)
    if (e0_) (void)hipEventDestroy(e0_);
    if (e1_) (void)hipEventDestroy(e1_);
  }
  int open(int device, void* stream) {
    guard_.emplace(device);
    s = (hipStream_t)stream;
    fence_ = fence_mode_from_env();      // POSERISK_FENCE, per call: the entry's own copies between guards (fence.h)
    return refuse_if_capturing(s, "stand-alone test entry");   // allocates and synchronises: never inside a capture
  }
  // `name`: what the internal fence records the buffer under ("standalone <name>"); frame_bytes: one frame of it, if it has frames
  template <typename T>
  T* device_alloc(size_t count, const char* name, size_t frame_bytes = 0) {
    void* p = nullptr;
    if (st_ == PR_OK) st_ = alloc(count * sizeof(T), &p, name, frame_bytes);
    return (T*)p;
  }
  template <typename T>
  T* upload(const T* host, size_t count, const char* name) {      // nothing to upload (null or empty): null
    T* p = host && count ? device_alloc<T>(count, name) : nullptr;
    if (p) st_ = copy(p, host, count * sizeof(T));
    return st_ == PR_OK ? p : nullptr;
  }
  template <typename T>
  T* upload(const std::vector<T>& v, const char* name) { return upload(v.data(), v.size(), name); }
  // launch once; with repeats > 0 and ms_out, `repeats` more between two events (*ms_out = milliseconds per launch)
  template <typename Launch>
  int run(Launch launch, int repeats = 0, float* ms_out = nullptr) {
    PR_TRY(st_);
    int st = launch();
    if (st == PR_OK && repeats > 0 && ms_out) {
      PR_HIP(hipEventCreate(&e0_));
      PR_HIP(hipEventCreate(&e1_));
      PR_HIP(hipEventRecord(e0_, s));
      for (int i = 0; i < repeats && st == PR_OK; ++i) st = launch();
      PR_HIP(hipEventRecord(e1_, s));
      PR_HIP(hipEventSynchronize(e1_));
      float ms = 0.f;
      PR_HIP(hipEventElapsedTime(&ms, e0_, e1_));
      *ms_out = ms / repeats;
    }
    const hipError_t e = hipStreamSynchronize(s);  // the buffers must outlive the launches
    if (st != PR_OK) return st;                    // the kernel's status first, then the synchronisation's
    PR_HIP(e);
    return PR_OK;
  }

 private:
  int alloc(size_t bytes, void** p, const char* name, size_t frame_bytes) {
    PR_TRY(pr::device_alloc(p, bytes, fence_, frame_bytes, "standalone %s", name));
    bufs_.push_back(*p);
    return PR_OK;
  }
  int copy(void* dst, const void* host, size_t bytes) {
    PR_HIP(hipMemcpy(dst, host, bytes, hipMemcpyHostToDevice));
    return PR_OK;
  }
  std::optional<DeviceGuard> guard_;      // outlives the destructor's body: the buffers are freed on the device they are on
  std::vector<void*> bufs_;
  hipEvent_t e0_ = nullptr, e1_ = nullptr;
  int st_ = PR_OK;
  int fence_ = 0;
};

// The three whole-Bottleneck entries behind their argument checks: w / b = conv1, conv2, conv3, the downsample branch (or null)
int bottleneck_entry(int planes, int device, const void* x_dev, const float* const w[4], const float* const b[4], void* y_dev,
                     int B, int H, int W, int repeats, float* ms_out, void* stream) {
  StandAlone sa;
  PR_TRY(sa.open(device, stream));
  const int couts[4] = {planes, planes, 4 * planes, 4 * planes};
  std::vector<double> bias[4];
  ConvFilter f[4];
  for (int i = 0; i < 4; ++i)
    if (w[i]) {
      bias[i].assign(b[i], b[i] + couts[i]);
      f[i] = ConvFilter{w[i], nullptr, bias[i].data()};
    }
  BottleneckWeights bw;      // the layouts the encoder's plan uploads (host_plan.cc)
  PR_TRY(bottleneck_pack_bf16(planes, f[0], f[1], f[2], w[3] ? &f[3] : nullptr, &bw));
  BottleneckProblem p;
  p.x = x_dev; p.y = y_dev; p.w1 = sa.upload(bw.w1, "block w1"); p.w2 = sa.upload(bw.w2, "block w2"); p.w3 = sa.upload(bw.w3, "block w3");
  p.b1 = sa.upload(bw.b1, "block b1"); p.b2 = sa.upload(bw.b2, "block b2"); p.b3 = sa.upload(bw.b3, "block b3");
  p.B = B; p.H = H; p.W = W; p.planes = planes; p.first = w[3] != nullptr;
  return sa.run([&] { return bottleneck_bf16_launch(p, sa.s); }, repeats, ms_out);
}

}  // namespace
}  // namespace pr

extern "C" {

int pr_conv2d_nhwc(int device, const void* x_dev, const float* w_host, const float* bias_host,
                   const void* res_dev, void* y_dev, int B, int H, int W, int Cin, int Cin_real, int Cout,
                   int KH, int KW, int stride, int pad, int relu, int tile_cfg, int precision, int repeats,
                   float* ms_out, void* stream) {
  using namespace pr;
  PR_REQUIRE(x_dev && w_host && y_dev, "pr_conv2d_nhwc: null argument");
  PR_REQUIRE(precision == 0 || precision == 1, "pr_conv2d_nhwc: precision %d unknown", precision);
  PR_REQUIRE(precision == 0 || Cin % 8 == 0, "pr_conv2d_nhwc: bf16 needs Cin %% 8 == 0");
  PR_REQUIRE(Cin_real > 0 && Cin_real <= Cin && Cout % 64 == 0, "pr_conv2d_nhwc: bad channels");
  PR_REQUIRE(stride > 0 && pad >= 0 && KH > 0 && KW > 0, "pr_conv2d_nhwc: bad geometry");
  StandAlone sa;
  PR_TRY(sa.open(device, stream));
  ConvProblem p;
  p.B = B; p.H = H; p.W = W; p.Cin = Cin; p.Cout = Cout; p.KH = KH; p.KW = KW; p.stride = stride; p.pad = pad;
  p.Ho = (H + 2 * pad - KH) / stride + 1;
  p.Wo = (W + 2 * pad - KW) / stride + 1;
  p.relu = relu;
  PR_REQUIRE(p.Ho > 0 && p.Wo > 0, "pr_conv2d_nhwc: empty output");
  p.precision = precision;
  p.tune = conv_tuning_from_env();
  const float* wd = nullptr;
  float* work = nullptr;
  const bool wino = tile_cfg == -2 || tile_cfg == -4 || tile_cfg == -5;
  const int wino_m = -tile_cfg;      // the Winograd form (2, 4, 5)
  if (wino) {
    PR_REQUIRE(precision == 0 && KH == 3 && KW == 3 && stride == 1 && pad == 1 && !res_dev && Cin == Cin_real &&
                   Cin % 32 == 0,
               "pr_conv2d_nhwc: tile_cfg -2 / -4 / -5 (Winograd) is for fp32 3x3 / stride 1 / pad 1 without residual, Cin %% 32 == 0");
    const int wn = conv_winograd_tile(wino_m) + 2;
    std::vector<float> u((size_t)wn * wn * Cout * Cin);
    conv_winograd_pack_weights(w_host, nullptr, Cout, Cin, wino_m, u.data());
    wd = sa.upload(u, "u");
    work = sa.device_alloc<float>(std::max<size_t>(conv_winograd_work_floats(p, wino_m), 4), "wino_work",
                                  B > 0 ? conv_winograd_work_floats(p, wino_m) / B * sizeof(float) : 0);
  } else if (precision == 1) {      // KH x KW may differ here, so the row packers and not conv_pack_side_by_side
    std::vector<unsigned short> packed((size_t)Cout * conv_kpad_bf16(p.K()));
    conv_pack_weights_bf16(w_host, nullptr, Cout, Cin_real, Cin, KH, KW, packed.data());
    wd = (const float*)sa.upload(packed, "weights");
  } else {
    std::vector<float> packed((size_t)Cout * p.Kpad());
    conv_pack_weights(w_host, nullptr, Cout, Cin_real, Cin, KH, KW, packed.data());
    wd = sa.upload(packed, "weights");
  }
  p.x = (const float*)x_dev; p.w = wd; p.bias = sa.upload(bias_host, Cout, "bias"); p.res = (const float*)res_dev; p.y = (float*)y_dev;
  int cfg = tile_cfg >= 0 ? tile_cfg : conv_pick_tile_cfg(p.shape(), p.tune);
  if (tile_cfg > 200 && tile_cfg <= 208) {      // 64x64 tile with the K-steps of every tile dealt to tile_cfg - 200 workgroups
    PR_REQUIRE(precision == 0, "pr_conv2d_nhwc: split-K is fp32 only");
    cfg = 8;
    p.splitk = tile_cfg - 200;
    const size_t tiles = (size_t)ceil_div(p.M(), 64) * (Cout / 64);
    p.split_slab = sa.device_alloc<float>(tiles * p.splitk * 4096, "split_slab");
    p.split_tickets = sa.device_alloc<int>(tiles, "split_tickets");
  }
  return sa.run([&] { return wino ? conv_winograd_launch(p, wd, work, wino_m, sa.s) : conv_launch(p, cfg, sa.s); }, repeats, ms_out);
}

int pr_conv1x1_dual_nhwc(int device, const void* x1_dev, const float* w1_host, const void* x2_dev, const float* w2_host,
                         const float* bias_host, void* y_dev, int B, int Ho, int Wo, int Cin1, int H2, int W2, int Cin2,
                         int stride2, int Cout, int relu, int tile_cfg, int precision, void* stream) {
  using namespace pr;
  PR_REQUIRE(x1_dev && w1_host && x2_dev && w2_host && y_dev, "pr_conv1x1_dual_nhwc: null argument");
  PR_REQUIRE(precision == 0 || precision == 1, "pr_conv1x1_dual_nhwc: precision %d unknown", precision);
  const int kq = precision == 1 ? 64 : kConvBK;
  PR_REQUIRE(Cin1 > 0 && Cin2 > 0 && Cin1 % kq == 0 && Cin2 % kq == 0 && Cout % 64 == 0 && stride2 > 0,
             "pr_conv1x1_dual_nhwc: channels must be multiples of %d (Cout of 64)", kq);
  StandAlone sa;
  PR_TRY(sa.open(device, stream));
  ConvProblem p;
  p.B = B; p.H = p.Ho = Ho; p.W = p.Wo = Wo; p.Cin = Cin1; p.Cout = Cout; p.KH = p.KW = 1; p.stride = 1; p.pad = 0;
  p.relu = relu; p.precision = precision;
  p.tune = conv_tuning_from_env();
  p.H2 = H2; p.W2 = W2; p.Cin2 = Cin2; p.stride2 = stride2;
  const ConvFilter f1{w1_host}, f2{w2_host};
  p.w = sa.upload(conv_pack_side_by_side(f1, Cin1, Cin1, 1, &f2, Cin2, Cout, precision), "dual weights");
  p.x = (const float*)x1_dev; p.x2 = (const float*)x2_dev; p.bias = sa.upload(bias_host, Cout, "bias"); p.res = nullptr; p.y = (float*)y_dev;
  const int cfg = tile_cfg >= 0 ? tile_cfg : conv_pick_tile_cfg(p.shape(), p.tune);
  return sa.run([&] { return conv_launch(p, cfg, sa.s); });
}

int pr_conv3x3_conv1x1_nhwc(int device, const void* x_dev, const float* w2_host, const float* b2_host,
                            const float* w3_host, const float* b3_host, const void* res_dev, void* y_dev, int B, int H,
                            int W, int Cin, int N3, int relu3, int precision, void* stream) {
  using namespace pr;
  PR_REQUIRE(x_dev && w2_host && b2_host && w3_host && b3_host && y_dev, "pr_conv3x3_conv1x1_nhwc: null argument");
  PR_REQUIRE(precision == 0 || precision == 1, "pr_conv3x3_conv1x1_nhwc: precision %d unknown", precision);
  PR_REQUIRE(Cin >= (precision ? 64 : 32) && (Cin & (Cin - 1)) == 0 && N3 > 0 && N3 % 64 == 0,
             "pr_conv3x3_conv1x1_nhwc: Cin must be a power of two >= 32 (bf16: 64), N3 a multiple of 64");
  StandAlone sa;
  PR_TRY(sa.open(device, stream));
  ConvProblem p;
  p.B = B; p.H = p.Ho = H; p.W = p.Wo = W; p.Cin = Cin; p.Cout = 64; p.KH = p.KW = 3; p.stride = 1; p.pad = 1; p.relu = 1;
  p.precision = precision;
  p.tune = conv_tuning_from_env();
  p.x = (const float*)x_dev;
  p.w = sa.upload(conv_pack_side_by_side(ConvFilter{w2_host}, Cin, Cin, 3, nullptr, 0, 64, precision), "conv2 weights");
  p.bias = sa.upload(b2_host, 64, "conv2 bias");
  p.w3 = sa.upload(conv_pack_side_by_side(ConvFilter{w3_host}, 64, 64, 1, nullptr, 0, N3, precision), "conv3 weights");
  p.bias3 = sa.upload(b3_host, N3, "conv3 bias");
  p.res3 = (const float*)res_dev; p.y3 = (float*)y_dev;
  p.N3 = N3; p.relu3 = relu3;
  return sa.run([&] { return conv_launch(p, 8, sa.s); });
}

int pr_conv3x3_wino64_nhwc(int device, const void* x_dev, const float* w2_host, const float* b2_host, const float* w3_host,
                           const float* b3_host, const void* res_dev, void* y_dev, int B, int H, int W, int Cin, int Cout, int N3,
                           int relu2, int relu3, int form, void* stream) {
  using namespace pr;
  PR_REQUIRE(x_dev && w2_host && b2_host && y_dev, "pr_conv3x3_wino64_nhwc: null argument");
  PR_REQUIRE(Cin == 64 && Cout == 64, "pr_conv3x3_wino64_nhwc: Cin = Cout = 64 only (got %d -> %d)", Cin, Cout);
  PR_REQUIRE(form == 4 || form == 5, "pr_conv3x3_wino64_nhwc: form %d is not 4 or 5", form);
  PR_REQUIRE(B >= 0 && H > 0 && W > 0, "pr_conv3x3_wino64_nhwc: bad geometry");
  PR_REQUIRE(!w3_host || (b3_host && N3 > 0 && N3 % 64 == 0), "pr_conv3x3_wino64_nhwc: conv3 needs a bias and N3 %% 64 == 0 (%d)", N3);
  StandAlone sa;
  PR_TRY(sa.open(device, stream));
  std::vector<float> u((size_t)36 * 64 * 64), up(u.size());
  conv_winograd_pack_weights(w2_host, nullptr, 64, 64, form, u.data());
  conv_wino64_pack_u(u.data(), up.data());
  const float* ud = sa.upload(up, "u1");
  ConvProblem p;
  p.B = B; p.H = p.Ho = H; p.W = p.Wo = W; p.Cin = 64; p.Cout = 64; p.KH = p.KW = 3; p.stride = 1; p.pad = 1; p.relu = relu2;
  p.precision = 0;
  p.x = (const float*)x_dev; p.w = nullptr; p.bias = sa.upload(b2_host, 64, "conv2 bias"); p.res = nullptr; p.y = w3_host ? nullptr : (float*)y_dev;
  if (w3_host) {
    p.w3 = sa.upload(w3_host, (size_t)N3 * 64, "conv3 weights"); p.bias3 = sa.upload(b3_host, N3, "conv3 bias");
    p.res3 = (const float*)res_dev; p.y3 = (float*)y_dev; p.N3 = N3; p.relu3 = relu3;
  }
  return sa.run([&] { return conv_wino64_launch(p, ud, form, sa.s); });
}

int pr_bottleneck_nhwc(int device, const void* x_dev, const float* w1_host, const float* b1_host, const float* w2_host,
                       const float* b2_host, const float* w3_host, const float* b3_host, const float* wd_host,
                       const float* bd_host, void* y_dev, int B, int H, int W, int repeats, float* ms_out, void* stream) {
  PR_REQUIRE(x_dev && w1_host && b1_host && w2_host && b2_host && w3_host && b3_host && y_dev, "pr_bottleneck_nhwc: null argument");
  PR_REQUIRE(!wd_host == !bd_host, "pr_bottleneck_nhwc: the downsample branch needs both its weight and its bias");
  PR_REQUIRE(B >= 0 && H > 0 && W > 0, "pr_bottleneck_nhwc: bad geometry");
  const float *const w[4] = {w1_host, w2_host, w3_host, wd_host}, *const b[4] = {b1_host, b2_host, b3_host, bd_host};
  return pr::bottleneck_entry(64, device, x_dev, w, b, y_dev, B, H, W, repeats, ms_out, stream);
}

int pr_bottleneck128_nhwc(int device, const void* x_dev, const float* w1_host, const float* b1_host, const float* w2_host,
                          const float* b2_host, const float* w3_host, const float* b3_host, void* y_dev, int B, int H, int W,
                          int repeats, float* ms_out, void* stream) {
  PR_REQUIRE(x_dev && w1_host && b1_host && w2_host && b2_host && w3_host && b3_host && y_dev, "pr_bottleneck128_nhwc: null argument");
  PR_REQUIRE(B >= 0 && H > 0 && W > 0, "pr_bottleneck128_nhwc: bad geometry");
  const float *const w[4] = {w1_host, w2_host, w3_host, nullptr}, *const b[4] = {b1_host, b2_host, b3_host, nullptr};
  return pr::bottleneck_entry(128, device, x_dev, w, b, y_dev, B, H, W, repeats, ms_out, stream);
}

int pr_bottleneck256_nhwc(int device, const void* x_dev, const float* w1_host, const float* b1_host, const float* w2_host,
                          const float* b2_host, const float* w3_host, const float* b3_host, void* y_dev, int B, int H, int W,
                          int repeats, float* ms_out, void* stream) {
  PR_REQUIRE(x_dev && w1_host && b1_host && w2_host && b2_host && w3_host && b3_host && y_dev, "pr_bottleneck256_nhwc: null argument");
  PR_REQUIRE(B >= 0 && H > 0 && W > 0, "pr_bottleneck256_nhwc: bad geometry");
  const float *const w[4] = {w1_host, w2_host, w3_host, nullptr}, *const b[4] = {b1_host, b2_host, b3_host, nullptr};
  return pr::bottleneck_entry(256, device, x_dev, w, b, y_dev, B, H, W, repeats, ms_out, stream);
}

int pr_stem_pool_nhwc(int device, const void* x_dev, const float* w_host, const float* bias_host, void* y_dev, int B, int H,
                      int repeats, float* ms_out, void* stream) {
  using namespace pr;
  PR_REQUIRE(x_dev && w_host && bias_host && y_dev, "pr_stem_pool_nhwc: null argument");
  StandAlone sa;
  PR_TRY(sa.open(device, stream));
  const float* wd = sa.upload(conv_pack_side_by_side(ConvFilter{w_host}, 16, 16, 4, nullptr, 0, 64, 1), "stem weights");      // k = (th * 4 + tw) * 16 + c
  const float* bd = sa.upload(bias_host, 64, "stem bias");
  return sa.run([&] { return stem_pool_bf16_launch(x_dev, wd, bd, y_dev, B, H, sa.s); }, repeats, ms_out);
}

int pr_stem_pool_f32_nhwc(int device, const float* x_dev, const float* w_host, const float* bias_host, float* y_dev, int B,
                          int repeats, float* ms_out, void* stream) {
  using namespace pr;
  PR_REQUIRE(x_dev && w_host && bias_host && y_dev, "pr_stem_pool_f32_nhwc: null argument");
  StandAlone sa;
  PR_TRY(sa.open(device, stream));
  // the kernel shares MFMAs between the half-empty taps of the 7x7 kernel's zero row / column (stem_pool_f32.hip): weights
  // that are not a 7x7 kernel in the 8x8 window would be computed wrong, so they are refused
  for (int o = 0; o < 64; ++o)
    for (int c12 = 0; c12 < 12; ++c12)
      for (int t = 0; t < 4; ++t) {
        const int sub = c12 / 3;                                              // 2 di + dj
        const float top = w_host[((o * 12 + c12) * 4 + 0) * 4 + t], left = w_host[((o * 12 + c12) * 4 + t) * 4 + 0];
        PR_REQUIRE(((sub >> 1) != 0 || top == 0.f) && ((sub & 1) != 0 || left == 0.f),
                   "pr_stem_pool_f32_nhwc: the weights must be a 7x7 kernel in the 4x4 taps' 8x8 window (zero for tap row 0 / "
                   "sub-row 0 and for tap column 0 / sub-column 0); output channel %d, channel %d is not", o, c12);
      }
  const float* wd = sa.upload(conv_pack_side_by_side(ConvFilter{w_host}, 12, 12, 4, nullptr, 0, 64, 0), "stem weights");      // k = (th * 4 + tw) * 12 + c
  const float* bd = sa.upload(bias_host, 64, "stem bias");
  return sa.run([&] { return stem_pool_f32_launch(x_dev, wd, bd, y_dev, B, sa.s); }, repeats, ms_out);
}

int pr_frames_forward(pr_hmr_t* hmr, pr_smpl_t* smpl, const float* x_dev, int B,
                      const pr_reba_info* reba_info, const pr_rula_info* rula_info,
                      const pr_frames_out* out, void* stream) {
  PR_REQUIRE(B >= 0, "pr_frames_forward: negative batch");
  if (B == 0) return PR_OK;  // an empty batch is legal (empty tensors have null data pointers)
  PR_REQUIRE(hmr && smpl && x_dev && out, "pr_frames_forward: null argument");
  PR_REQUIRE(out->rotmat && out->axis_angle && out->euler_deg && out->joint_cam,
             "pr_frames_forward: rotmat, axis_angle, euler_deg and joint_cam are required");
  PR_REQUIRE((!out->reba || reba_info) && (!out->rula || rula_info), "pr_frames_forward: score output without info");
  // base.py:220        encoder + regressor
  PR_TRY(pr_hmr_forward(hmr, x_dev, B, out->rotmat, out->betas, out->cam, nullptr, nullptr, stream));
  // base.py:225-229    rotmat -> axis-angle -> Euler degrees (per frame, per joint)
  PR_TRY(pr_pose_to_euler(out->rotmat, B, out->axis_angle, out->euler_deg, out->status, stream));
  // base.py:239        joint_cam (mutates axis_angle's root rows, as the reference does)
  PR_TRY(pr_smpl_joint_cam(smpl, out->axis_angle, B, out->joint_cam, out->verts, stream));
  // base.py:151,168    scorers
  if (out->reba) PR_TRY(pr_reba(out->euler_deg, B, reba_info, out->reba, stream));
  if (out->rula) PR_TRY(pr_rula(out->euler_deg, B, rula_info, out->rula, stream));
  return PR_OK;
}

}  // extern "C"
