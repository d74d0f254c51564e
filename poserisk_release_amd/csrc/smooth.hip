// Temporal smoothing of each track's poses: pr_smooth_tracks.  The contract -- groups, windows on frame numbers, the medoid
// of stage 1, the Gaussian and the polar factor of stage 2, the fallback -- is written in include/poserisk_hip.h (section s1);
// tests/smooth_ref.py restates it in float64 numpy, tests/test_smooth_native.py runs this file on the host under sanitizers,
// tests/test_smooth_gpu.py runs it on the GPU between guard bands.
//
// One kernel, launched once per stage.  A workgroup takes kTileRows consecutive rows and stages them, with `radius` rows of
// halo on each side (clamped to the launch's rows), in LDS once: whole rows, rotmat | cam | betas, 229 floats, with their
// frame numbers.  It then works the tile's (row, group) items, row fastest, so that the lanes of a wave walk windows of the
// same length and read LDS at an odd stride (229 dwords: no two lanes of a row-run share a bank).  Everything after the
// staging reads LDS only: without it every input row would be read again by up to 31 rows' windows.
//
// The tracks' bounds travel in the kernel's arguments (kMaxTracks + 1 ints), so the host array needs no copy to the device and
// the entry stays capturable; more tracks than that take one pair of launches per kMaxTracks tracks, which is exact because
// a window never crosses a track boundary.
//
// All arithmetic of the contract is float64 with contraction off: stage 1's costs decide an argmin whose exact ties the
// contract breaks by rule, so a cost has to be the same number here, on the host build and in the numpy restatement.
#include <cmath>

#include "common.h"

namespace pr {
namespace {

constexpr int kThreads = 256;
constexpr int kTileRows = 32;
constexpr int kMaxRadius = PR_SMOOTH_MAX_RADIUS;
constexpr int kMaxTracks = PR_SMOOTH_TRACKS_PER_LAUNCH;
constexpr int kLdsRows = kTileRows + 2 * kMaxRadius;
constexpr int kRotFloats = 216, kCamFloats = 3, kBetaFloats = 10;
constexpr int kRowFloats = kRotFloats + kCamFloats + kBetaFloats;   // an LDS row: rotmat | cam | betas
constexpr int kGroups = 26;                                         // 24 joints, cam, betas
constexpr int kMaxRows = 1 << 23;                                   // N at most: every element index stays below 2^31
constexpr double kFallbackC = 0.05;
static_assert(kLdsRows * kRowFloats * 4 + (kLdsRows + 4 * kTileRows) * 4 <= 64 * 1024, "the tile fits the default LDS limit");

struct Params {
  const float* in[3];   // rotmat, cam, betas (null: absent)
  float* out[3];
  const int32_t* frame_no;
  int32_t* status;      // written (bits of stage 2, or 0) where not null
  int32_t* replaced;    // written (bits of stage 1, or 0) where not null
  double sigma;
  int stage;            // 1: medoid, 2: Gaussian
  int radius;
  int row0, row1;       // the rows of this launch: those of its n_tracks tracks
  int n_tracks;
  int start[kMaxTracks + 1];   // start[0] = row0 <= ... <= start[n_tracks] = row1
};

__device__ __forceinline__ int tensor_width(int t) { return t == 0 ? kRotFloats : t == 1 ? kCamFloats : kBetaFloats; }
__device__ __forceinline__ int tensor_offset(int t) { return t == 0 ? 0 : t == 1 ? kRotFloats : kRotFloats + kCamFloats; }

__device__ __forceinline__ double det3(const double* m) {
#pragma clang fp contract(off)
  return m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6]) + m[2] * (m[3] * m[7] - m[4] * m[6]);
}

// A = sum w Y -> the orthogonal polar factor of A in R; false (R untouched) where c < kFallbackC or c is not a number.
__device__ inline bool polar_factor(const double* A, double* R) {
#pragma clang fp contract(off)
  double fro2 = 0.0;
  for (int e = 0; e < 9; ++e) fro2 += A[e] * A[e];
  const double s = sqrt(fro2) / sqrt(3.0);
  const double c = det3(A) / (s * s * s);
  if (!(c >= kFallbackC)) return false;
  double X[9];
  for (int e = 0; e < 9; ++e) X[e] = A[e] / s;
  // scaled Newton: X <- (mu X + X^-T / mu) / 2, mu = |det X|^(-1/3).  c >= 0.05 bounds the condition number, the iteration
  // converges quadratically; 32 steps are never reached (about 6 at c = 0.05).
  for (int it = 0; it < 32; ++it) {
    const double C[9] = {X[4] * X[8] - X[5] * X[7], X[5] * X[6] - X[3] * X[8], X[3] * X[7] - X[4] * X[6],
                         X[2] * X[7] - X[1] * X[8], X[0] * X[8] - X[2] * X[6], X[1] * X[6] - X[0] * X[7],
                         X[1] * X[5] - X[2] * X[4], X[2] * X[3] - X[0] * X[5], X[0] * X[4] - X[1] * X[3]};   // cofactors = det X^-T
    const double d = X[0] * C[0] + X[1] * C[1] + X[2] * C[2];
    const double mu = 1.0 / cbrt(fabs(d));
    const double a = 0.5 * mu, b = 0.5 / (mu * d);
    double delta = 0.0;
    for (int e = 0; e < 9; ++e) {
      const double n = a * X[e] + b * C[e];
      delta = fmax(delta, fabs(n - X[e]));
      X[e] = n;
    }
    if (delta <= 1e-14) break;
  }
  for (int e = 0; e < 9; ++e) R[e] = X[e];
  return true;
}

__global__ void __launch_bounds__(kThreads) smooth_kernel(Params p) {
#pragma clang fp contract(off)
  __shared__ float tile[kLdsRows * kRowFloats];
  __shared__ int fno[kLdsRows];
  __shared__ int lo_s[kTileRows], hi_s[kTileRows];   // the bounds of each tile row's track
  __shared__ int fell[kTileRows], repl[kTileRows];   // status and replaced bits
  const int tid = (int)threadIdx.x;
  const int r = p.radius;
  const int a = p.row0 + (int)blockIdx.x * kTileRows, b = min(a + kTileRows, p.row1);
  const int h0 = max(a - r, p.row0), h1 = min(b + r, p.row1);      // the staged rows: h1 - h0 <= kLdsRows
  for (int t = 0; t < 3; ++t) {
    if (!p.in[t]) continue;
    const int w = tensor_width(t), off = tensor_offset(t);
    const float* src = p.in[t] + (size_t)h0 * w;
    for (int idx = tid; idx < (h1 - h0) * w; idx += kThreads) tile[(idx / w) * kRowFloats + off + idx % w] = src[idx];
  }
  for (int k = tid; k < h1 - h0; k += kThreads) fno[k] = p.frame_no[h0 + k];
  if (tid < b - a) {
    // the track of row i: the last one that starts at or before it and is not empty up to it
    const int i = a + tid;
    int lo = 0, hi = p.n_tracks;                 // start[lo] <= i < start[hi]
    while (hi - lo > 1) {
      const int mid = (lo + hi) / 2;
      if (p.start[mid] <= i) lo = mid; else hi = mid;
    }
    lo_s[tid] = p.start[lo];
    hi_s[tid] = p.start[hi];
    fell[tid] = 0;
    repl[tid] = 0;
  }
  __syncthreads();
  const int rows = b - a;
  for (int item = tid; item < rows * kGroups; item += kThreads) {
    const int row = item % rows, g = item / rows;
    const int t = g < 24 ? 0 : g - 23;
    if (!p.in[t]) continue;
    const int D = g < 24 ? 9 : tensor_width(t);
    const int off = g < 24 ? 9 * g : tensor_offset(t);
    const int i = a + row;
    const int k0 = max(i - r, lo_s[row]), k1 = min(i + r, hi_s[row] - 1);   // inside [h0, h1): lo >= row0, hi <= row1
    const long long fi = fno[i - h0];
    float* dst = p.out[t] + (size_t)i * tensor_width(t) + (g < 24 ? 9 * g : 0);
    if (p.stage == 1) {
      int best = i;
      double best_cost = 0.0;
      long long best_df = 0;
      bool have = false;
      for (int k = k0; k <= k1; ++k) {
        long long df = (long long)fno[k - h0] - fi;
        if (df < -r || df > r) continue;
        if (df < 0) df = -df;
        const float* xk = tile + (k - h0) * kRowFloats + off;
        double cost = 0.0;
        for (int l = k0; l <= k1; ++l) {
          const long long dl = (long long)fno[l - h0] - fi;
          if (dl < -r || dl > r) continue;
          const float* xl = tile + (l - h0) * kRowFloats + off;
          double ss = 0.0;
          for (int e = 0; e < D; ++e) {
            const double d = (double)xk[e] - (double)xl[e];
            ss = ss + d * d;
          }
          cost = cost + sqrt(ss);
        }
        if (!have || cost < best_cost || (cost == best_cost && df < best_df)) {
          have = true;
          best = k;
          best_cost = cost;
          best_df = df;
        }
      }
      const float* x = tile + (best - h0) * kRowFloats + off;
      for (int e = 0; e < D; ++e) dst[e] = x[e];
      if (best != i) atomicOr(&repl[row], 1 << g);
    } else {
      const double denom = 2.0 * p.sigma * p.sigma;
      double acc[10], wsum = 0.0;
      int count = 0;
      for (int e = 0; e < D; ++e) acc[e] = 0.0;
      for (int k = k0; k <= k1; ++k) {
        const long long df = (long long)fno[k - h0] - fi;
        if (df < -r || df > r) continue;
        const double w = df == 0 ? 1.0 : exp(-(double)(df * df) / denom);   // (a sigma whose square underflows: 1, then 0)
        const float* y = tile + (k - h0) * kRowFloats + off;
        for (int e = 0; e < D; ++e) acc[e] = acc[e] + w * (double)y[e];
        wsum = wsum + w;
        ++count;
      }
      if (count == 1) {   // an isolated row comes back as it is: the bits of y_i, not the rotation nearest to them
        const float* y = tile + (i - h0) * kRowFloats + off;
        for (int e = 0; e < D; ++e) dst[e] = y[e];
      } else if (g < 24) {
        double R[9];
        if (polar_factor(acc, R)) {
          for (int e = 0; e < 9; ++e) dst[e] = (float)R[e];
        } else {
          const float* y = tile + (i - h0) * kRowFloats + off;
          for (int e = 0; e < 9; ++e) dst[e] = y[e];
          atomicOr(&fell[row], 1 << g);
        }
      } else {
        for (int e = 0; e < D; ++e) dst[e] = (float)(acc[e] / wsum);
      }
    }
  }
  __syncthreads();
  if (tid < rows) {
    if (p.status) p.status[a + tid] = fell[tid];
    if (p.replaced) p.replaced[a + tid] = repl[tid];
  }
}

size_t workspace_bytes(int N, bool betas, bool cam) {
  const size_t floats = (size_t)N * (kRotFloats + (cam ? kCamFloats : 0) + (betas ? kBetaFloats : 0));
  return (floats * 4 + 255) / 256 * 256;
}

}  // namespace
}  // namespace pr

extern "C" int pr_smooth_tile_rows(void) { return pr::kTileRows; }

extern "C" size_t pr_smooth_workspace_bytes(int N, int has_betas, int has_cam) {
  return N < 0 ? 0 : pr::workspace_bytes(N, has_betas != 0, has_cam != 0);
}

extern "C" int pr_smooth_tracks(const pr_smooth_params* params, const pr_smooth_inputs* inputs, const int32_t* frame_no_dev,
                                const int* track_start_host, int T, int N, const pr_smooth_outputs* outputs, int32_t* status_dev,
                                void* workspace_dev, void* stream) {
  using namespace pr;
  PR_REQUIRE(params && inputs && outputs, "pr_smooth_tracks: null params, inputs or outputs");
  const int m = params->median_radius;
  const double sigma = params->sigma;
  PR_REQUIRE(m >= 0 && m <= kMaxRadius, "pr_smooth_tracks: median_radius = %d outside 0..%d", m, kMaxRadius);
  PR_REQUIRE(std::isfinite(sigma) && sigma >= 0.0, "pr_smooth_tracks: sigma = %g is not a finite number >= 0", sigma);
  PR_REQUIRE(params->reserved == 0, "pr_smooth_tracks: reserved = %d, not 0", params->reserved);
  PR_REQUIRE(N >= 0 && N <= kMaxRows, "pr_smooth_tracks: N = %d outside 0..%d", N, kMaxRows);
  PR_REQUIRE(T >= 0, "pr_smooth_tracks: T = %d", T);
  PR_REQUIRE(track_start_host, "pr_smooth_tracks: null track_start");
  PR_REQUIRE(track_start_host[0] == 0, "pr_smooth_tracks: track_start[0] = %d, not 0", track_start_host[0]);
  for (int t = 0; t < T; ++t)
    PR_REQUIRE(track_start_host[t] <= track_start_host[t + 1], "pr_smooth_tracks: track_start[%d] = %d > track_start[%d] = %d", t,
               track_start_host[t], t + 1, track_start_host[t + 1]);
  PR_REQUIRE(track_start_host[T] == N, "pr_smooth_tracks: track_start[T = %d] = %d, not N = %d", T, track_start_host[T], N);
  if (N == 0) return PR_OK;
  const int g = sigma > 0.0 ? (int)std::fmin(std::ceil(3.0 * sigma), (double)kMaxRadius) : 0;
  const bool stage1 = m > 0, stage2 = sigma > 0.0;
  PR_REQUIRE(inputs->rotmat && outputs->rotmat && frame_no_dev, "pr_smooth_tracks: null rotmat or frame_no");
  PR_REQUIRE(!inputs->betas == !outputs->betas, "pr_smooth_tracks: betas given on one side only");
  PR_REQUIRE(!inputs->cam == !outputs->cam, "pr_smooth_tracks: cam given on one side only");
  PR_REQUIRE(!(stage1 && stage2) || workspace_dev, "pr_smooth_tracks: null workspace with both stages");
  {
    // no output may be an input, another output or the workspace
    const void* ins[] = {inputs->rotmat, inputs->betas, inputs->cam, frame_no_dev};
    const void* outs[] = {outputs->rotmat, outputs->betas, outputs->cam, outputs->replaced, status_dev, workspace_dev};
    for (size_t o = 0; o < sizeof outs / sizeof outs[0]; ++o) {
      if (!outs[o]) continue;
      for (const void* in : ins) PR_REQUIRE(outs[o] != in, "pr_smooth_tracks: an output, status or the workspace aliases an input");
      for (size_t q = 0; q < o; ++q) PR_REQUIRE(outs[o] != outs[q], "pr_smooth_tracks: two outputs share one pointer");
    }
  }
  PR_REQUIRE((uintptr_t)workspace_dev % 4 == 0, "pr_smooth_tracks: workspace not 4-byte aligned");
  float* ws = (float*)workspace_dev;
  float* ws_t[3] = {ws, inputs->cam ? ws + (size_t)N * kRotFloats : nullptr,
                    inputs->betas ? ws + (size_t)N * (kRotFloats + (inputs->cam ? kCamFloats : 0)) : nullptr};
  const float* in_t[3] = {inputs->rotmat, inputs->cam, inputs->betas};
  float* out_t[3] = {outputs->rotmat, outputs->cam, outputs->betas};
  hipStream_t s = (hipStream_t)stream;
  for (int t0 = 0; t0 < T; t0 += kMaxTracks) {
    const int t1 = std::min(t0 + kMaxTracks, T);
    Params p{};
    p.frame_no = frame_no_dev;
    p.sigma = sigma;
    p.row0 = track_start_host[t0];
    p.row1 = track_start_host[t1];
    p.n_tracks = t1 - t0;
    if (p.row1 == p.row0) continue;
    for (int t = t0; t <= t1; ++t) p.start[t - t0] = track_start_host[t];
    const dim3 grid((unsigned)ceil_div(p.row1 - p.row0, kTileRows)), block(kThreads);
    if (stage1 || !stage2) {   // with neither stage: radius 0, every window is the row itself and the launch copies
      p.stage = 1;
      p.radius = m;
      for (int t = 0; t < 3; ++t) {
        p.in[t] = in_t[t];
        p.out[t] = stage2 ? ws_t[t] : out_t[t];
      }
      p.replaced = outputs->replaced;
      p.status = stage2 ? nullptr : status_dev;
      hipLaunchKernelGGL(smooth_kernel, grid, block, 0, s, p);
      PR_TRY(check_launch("smooth_kernel (stage 1)"));
    }
    if (stage2) {
      p.stage = 2;
      p.radius = g;
      for (int t = 0; t < 3; ++t) {
        p.in[t] = stage1 ? ws_t[t] : in_t[t];
        p.out[t] = out_t[t];
      }
      p.replaced = stage1 ? nullptr : outputs->replaced;
      p.status = status_dev;
      hipLaunchKernelGGL(smooth_kernel, grid, block, 0, s, p);
      PR_TRY(check_launch("smooth_kernel (stage 2)"));
    }
  }
  return PR_OK;
}
