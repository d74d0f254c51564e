// REBA's activity score and RULA's muscle use from each track's motion: pr_activity_tracks.  The contract -- the scored
// joints, dot, the windows on frame numbers, the events of stage A, held / repeated / rapid of stage B, the spread of stage C --
// is written in include/poserisk_hip.h (section t1); tests/activity_ref.py restates it in float64 numpy,
// tests/test_activity_native.py runs this file on the host under sanitizers, tests/test_activity_gpu.py runs it on the GPU
// between guard bands.
//
// Three kernels, launched once each per kMaxTracks tracks (their bounds travel in the arguments, as in smooth.hip).
//
//   events_kernel  stage A.  A workgroup per track: all lanes stage kEventRows rows of the twelve scored joints in LDS (the
//                  next chunk's loads in flight meanwhile), lanes 0..11 then walk one chain each through them, the anchor
//                  in registers.  The walk is sequential by definition; one long track sets this kernel's time.
//   window_kernel  stage B, the hot one: N x 12 x H nine-term float64 dots.  A workgroup takes kTileRows consecutive rows; lane
//                  (row, b) owns joint b of one row, whose 9 values it keeps in registers as doubles (a wave = one joint of
//                  64 rows; twelve waves a tile, so that 16 384 rows give every SIMD three waves to switch between).  The rows
//                  from the tile's last one down to H rows before its first (not below the first tile row's track) pass
//                  through LDS in chunks of kChunkRows rows, NEWEST FIRST, converted to double once on the way in, so the
//                  lanes of a wave read the same row k at the same time (one LDS address per read: a broadcast) and the
//                  tile's own rows are picked up from the chunks that hold them.  H rows x 12 joints x 36 B do not fit LDS;
//                  a chunk does.  Newest first because every reason to stop shows early that way: a lane needs no dot once its
//                  joint has moved or its window has a hole, rapid's window is the R nearest rows, and a workgroup leaves the
//                  chunk loop when none of its lanes needs an older row (a flag in LDS read behind the chunk's barrier, so
//                  every lane takes the same number of barriers).
//   spread_kernel  stage C and the outputs: a lane per row ORs stage B's masks over the H rows after it.
//
// The dots need no contraction pragma: each product of two floats is exact in float64 (see the header).
#include <cmath>

#include "common.h"

namespace pr {
namespace {

constexpr int kThreads = 256;
constexpr int kTileRows = 64;
constexpr int kGroupJoints = 1;                      // window_kernel: a lane per row and joint, so that a few thousand rows
constexpr int kGroups = 12 / kGroupJoints;           // ... already give every SIMD several waves to switch between
constexpr int kWindowThreads = kTileRows * kGroups;
constexpr int kChunkRows = 32;
constexpr int kEventRows = 64;
constexpr int kSpreadRows = 8;
constexpr int kJoints = 12;
constexpr int kRowVals = kJoints * 9;                // the scored part of a row
constexpr int kEventLoads = (kEventRows * kRowVals + kThreads - 1) / kThreads;     // values a lane stages per chunk
constexpr int kChunkLoads = (kChunkRows * kRowVals + kWindowThreads - 1) / kWindowThreads;
constexpr int kGroupVals = kGroupJoints * 9;         // a lane's values ...
constexpr int kGroupPitch = (kGroupVals + 1) / 2 * 2;   // ... on 16-byte boundaries in window_kernel's chunk: 128-bit LDS reads
constexpr int kRowPitch = kGroups * kGroupPitch;
constexpr int kMaxHold = PR_ACTIVITY_MAX_HOLD;
constexpr int kMaxTracks = PR_ACTIVITY_TRACKS_PER_LAUNCH;
constexpr int kMaxRows = 1 << 23;                    // N at most: every element index stays below 2^31
constexpr int kMaskL = 0x0f0, kMaskR = 0xf00, kMaskB = 0x00f;
static_assert(kGroups * kGroupJoints == kJoints && kTileRows % kChunkRows == 0, "a lane per (row, kGroupJoints joints)");
static_assert(kEventRows < kThreads && kChunkRows <= kWindowThreads && kWindowThreads <= 1024, "a lane stages a chunk's frame number");
static_assert(kChunkRows * kRowPitch * 8 + (2 * kChunkRows + 3 * kTileRows + 2) * 4 <= 64 * 1024, "window_kernel fits the default LDS limit");
static_assert(kEventRows * kRowVals * 4 + (2 * kEventRows + 1) * 4 <= 64 * 1024, "events_kernel fits the default LDS limit");

struct Params {
  const float* rotmat;
  const int32_t* frame_no;
  int32_t* moved;       // workspace i32[N]: stage A
  int32_t* held_rep;    // workspace i32[N]: stage B's held | repeated << 16
  int32_t* rapid;       // workspace i32[N]
  int32_t* flags;       // i32[N,4]
  int32_t* adds;        // i32[N,4]
  double dot_static, dot_move, dot_rapid;
  int H, R, G, E;
  int row0, row1;       // the rows of this launch: those of its n_tracks tracks
  int n_tracks;
  int start[kMaxTracks + 1];   // start[0] = row0 <= ... <= start[n_tracks] = row1
};

__device__ __forceinline__ int joint_index(int b) {
  constexpr int index[kJoints] = {3, 12, 4, 5, 13, 16, 18, 20, 14, 17, 19, 21};
  return index[b];
}

// the first and the one-past-last row of the track of row i: the last track that starts at or before it
__device__ __forceinline__ void track_of(const Params& p, int i, int& first, int& end) {
  int lo = 0, hi = p.n_tracks;                 // start[lo] <= i < start[hi]
  while (hi - lo > 1) {
    const int mid = (lo + hi) / 2;
    if (p.start[mid] <= i) lo = mid; else hi = mid;
  }
  first = p.start[lo];
  end = p.start[hi];
}

// The scored values of rows c0 .. c0 + cn - 1 in the order (row, joint bit, element): value idx of that list from global memory.
__device__ __forceinline__ float scored_value(const Params& p, int c0, int idx) {
  const int v = idx % kRowVals;
  return p.rotmat[(size_t)(c0 + idx / kRowVals) * 216 + joint_index(v / 9) * 9 + v % 9];
}

__global__ void __launch_bounds__(kThreads) events_kernel(Params p) {
  __shared__ float rows[kEventRows * kRowVals];
  __shared__ int fno[kEventRows + 1];            // fno[0]: the row before the chunk
  __shared__ int mv[kEventRows];
  const int tid = (int)threadIdx.x;
  const int first = p.start[blockIdx.x], end = p.start[blockIdx.x + 1];
  double anchor[9];
  for (int e = 0; e < 9; ++e) anchor[e] = 0.0;
  // a chunk's values wait in registers while the chains walk the chunk before it: the loads' latency hides behind the walk
  float pre[kEventLoads];
  int pre_f = 0;
  auto prefetch = [&](int c0) {
    const int cn = min(kEventRows, end - c0);
#pragma unroll
    for (int u = 0; u < kEventLoads; ++u) {
      const int idx = tid + u * kThreads;
      pre[u] = idx < cn * kRowVals ? scored_value(p, c0, idx) : 0.f;
    }
    if (tid < cn) pre_f = p.frame_no[c0 + tid];
    if (tid == kEventRows) pre_f = c0 > first ? p.frame_no[c0 - 1] : 0;
  };
  if (first < end) prefetch(first);
  for (int c0 = first; c0 < end; c0 += kEventRows) {
    const int cn = min(kEventRows, end - c0);
#pragma unroll
    for (int u = 0; u < kEventLoads; ++u) {
      const int idx = tid + u * kThreads;
      if (idx < cn * kRowVals) rows[idx] = pre[u];
    }
    if (tid < cn) {
      fno[tid + 1] = pre_f;
      mv[tid] = 0;
    }
    if (tid == kEventRows) fno[0] = pre_f;
    __syncthreads();
    if (c0 + kEventRows < end) prefetch(c0 + kEventRows);
    if (tid < kJoints) {
      for (int kk = 0; kk < cn; ++kk) {
        const float* x = rows + kk * kRowVals + tid * 9;
        const long long step = (long long)fno[kk + 1] - (long long)fno[kk];
        bool take = c0 + kk == first || step > p.G || step < 0;
        if (!take) {
          double dot = anchor[0] * (double)x[0];
          for (int e = 1; e < 9; ++e) dot = dot + anchor[e] * (double)x[e];
          if (dot < p.dot_move) {
            atomicOr(&mv[kk], 1 << tid);
            take = true;
          }
        }
        if (take)
          for (int e = 0; e < 9; ++e) anchor[e] = (double)x[e];
      }
    }
    __syncthreads();
    if (tid < cn) p.moved[c0 + tid] = mv[tid];
    __syncthreads();                             // the next chunk overwrites rows, fno and mv
  }
}

__global__ void __launch_bounds__(kWindowThreads) window_kernel(Params p) {
  __shared__ __attribute__((aligned(16))) double chunk[kChunkRows * kRowPitch];
  __shared__ int fno[kChunkRows], mvd[kChunkRows];
  __shared__ int first_s[kTileRows], hr_s[kTileRows], rp_s[kTileRows];
  __shared__ int alive_s[2];
  const int tid = (int)threadIdx.x;
  const int row = tid % kTileRows, g = tid / kTileRows;
  const int a = p.row0 + (int)blockIdx.x * kTileRows, b = min(a + kTileRows, p.row1);
  const int H = p.H, R = p.R;
  if (tid < b - a) {
    int first, end;
    track_of(p, a + tid, first, end);
    first_s[tid] = first;
    hr_s[tid] = 0;
    rp_s[tid] = 0;
  }
  if (tid < 2) alive_s[tid] = 0;
  __syncthreads();
  const bool mine = row < b - a;
  const int i = a + row;
  const int k_first = mine ? max(i - H, first_s[row]) : 0;     // the lowest row of W_i(H), frame numbers aside
  const int lowest = max(a - H, first_s[0]);                   // ... of the whole tile: later rows' tracks start no earlier
  double Ri[kGroupVals];
  for (int e = 0; e < kGroupVals; ++e) Ri[e] = 0.0;
  long long fi = 0, f_prev = 0;                                // frame_no[i]; that of the lowest member seen so far
  bool covered = true;                                         // no hole among the members seen so far
  bool still[kGroupJoints], rapid[kGroupJoints];
  int count[kGroupJoints];
  for (int j = 0; j < kGroupJoints; ++j) {
    still[j] = true;
    rapid[j] = false;
    count[j] = 0;
  }
  const int n_chunks = (b - lowest + kChunkRows - 1) / kChunkRows;
  // the next (older) chunk's values wait in registers while this one is worked: the loads' latency hides behind the dots
  float pre[kChunkLoads];
  int pre_f = 0, pre_m = 0;
  auto prefetch = [&](int it) {
    const int c0 = lowest + (n_chunks - 1 - it) * kChunkRows, cn = min(kChunkRows, b - c0);
#pragma unroll
    for (int u = 0; u < kChunkLoads; ++u) {
      const int idx = tid + u * kWindowThreads;
      pre[u] = idx < cn * kRowVals ? scored_value(p, c0, idx) : 0.f;
    }
    if (tid < cn) {
      pre_f = p.frame_no[c0 + tid];
      pre_m = p.moved[c0 + tid];
    }
  };
  prefetch(0);
  for (int it = 0; it < n_chunks; ++it) {
    const int c0 = lowest + (n_chunks - 1 - it) * kChunkRows, cn = min(kChunkRows, b - c0);
    if (tid == 0) alive_s[it & 1] = 0;                         // last read two barriers ago
#pragma unroll
    for (int u = 0; u < kChunkLoads; ++u) {
      const int idx = tid + u * kWindowThreads, v = idx % kRowVals;
      if (idx < cn * kRowVals) chunk[(idx / kRowVals) * kRowPitch + (v / kGroupVals) * kGroupPitch + v % kGroupVals] = (double)pre[u];
    }
    if (tid < cn) {
      fno[tid] = pre_f;
      mvd[tid] = pre_m;
    }
    __syncthreads();
    if (it + 1 < n_chunks) prefetch(it + 1);                   // (read even where the loop then stops early: rows of the tile's windows)
    bool need = mine && i < c0;                                // my row lies in an older chunk
    const bool active = mine && i >= c0;
    if (active && i < c0 + cn) {                               // the chunk that holds my row: pick it up
      const double* mine_x = chunk + (i - c0) * kRowPitch + g * kGroupPitch;
      for (int e = 0; e < kGroupVals; ++e) Ri[e] = mine_x[e];
      fi = f_prev = fno[i - c0];
    }
    if (active) {
      for (int k = c0 + cn - 1; k >= c0; --k) {                // the same k in every lane of the wave: one LDS address
        if (k > i || k < k_first) continue;
        if (!covered && i - k > R) continue;                   // held and repeated are 0 and rapid's window is behind
        const long long fk = fno[k - c0], df = fi - fk;
        if (df < 0 || df > H) continue;                        // no member of W_i(H)
        if (k != i) {
          const long long step = f_prev - fk;
          if (step < 1 || step > p.G) covered = false;
        }
        f_prev = fk;
        const bool in_r = i - k <= R && df <= R;
        const int m = mvd[k - c0] >> (g * kGroupJoints);
        const double* x = chunk + (k - c0) * kRowPitch + g * kGroupPitch;
        for (int j = 0; j < kGroupJoints; ++j) {
          count[j] += m >> j & 1;
          if ((covered && still[j]) || (in_r && !rapid[j])) {
            double dot = x[9 * j] * Ri[9 * j];
            for (int e = 1; e < 9; ++e) dot = dot + x[9 * j + e] * Ri[9 * j + e];
            if (!(dot >= p.dot_static)) still[j] = false;
            if (in_r && dot < p.dot_rapid) rapid[j] = true;
          }
        }
      }
      need = c0 > k_first && (covered || i - c0 < R);          // row c0 - 1 can still change an output of mine
    }
    if (need) atomicOr(&alive_s[it & 1], 1);
    __syncthreads();
    if (!alive_s[it & 1]) break;                               // the same answer in every lane
  }
  if (mine) {
    // covered held all the way down, so f_prev is frame_no[p] of the window's first row p
    const bool whole = covered && fi - f_prev > (long long)H - (long long)p.G;
    int held = 0, repeated = 0, fast = 0;
    for (int j = 0; j < kGroupJoints; ++j) {
      const int bit = 1 << (g * kGroupJoints + j);
      if (whole && still[j]) held |= bit;
      if (whole && count[j] > p.E) repeated |= bit;
      if (rapid[j]) fast |= bit;
    }
    if (held | repeated) atomicOr(&hr_s[row], held | repeated << 16);
    if (fast) atomicOr(&rp_s[row], fast);
  }
  __syncthreads();
  if (tid < b - a) {
    p.held_rep[a + tid] = hr_s[tid];
    p.rapid[a + tid] = rp_s[tid];
  }
}

__global__ void __launch_bounds__(kThreads) spread_kernel(Params p) {
  const int i = p.row0 + (int)blockIdx.x * kThreads + (int)threadIdx.x;
  if (i >= p.row1) return;
  int first, end;
  track_of(p, i, first, end);
  const long long fi = p.frame_no[i];
  const int e_hi = min(i + p.H, end - 1);
  const int all = 0x0fff0fff;
  int acc = 0;
  for (int e0 = i; e0 <= e_hi && acc != all; e0 += kSpreadRows) {   // kSpreadRows independent loads in flight
    int f[kSpreadRows], m[kSpreadRows];
#pragma unroll
    for (int u = 0; u < kSpreadRows; ++u) {
      const int e = min(e0 + u, e_hi);                        // (past the end: the last row again, which an OR does not mind)
      f[u] = p.frame_no[e];
      m[u] = p.held_rep[e];
    }
#pragma unroll
    for (int u = 0; u < kSpreadRows; ++u) {
      const long long df = (long long)f[u] - fi;
      if (df >= 0 && df <= p.H) acc |= m[u];
    }
  }
  const int held = acc & 0xfff, repeated = acc >> 16 & 0xfff, fast = p.rapid[i], loaded = held | repeated;
  int32_t* f = p.flags + (size_t)i * 4;
  f[0] = held;
  f[1] = repeated;
  f[2] = fast;
  f[3] = p.moved[i];
  int32_t* o = p.adds + (size_t)i * 4;
  o[0] = (held != 0) + (repeated != 0) + (fast != 0);
  o[1] = (loaded & kMaskL) != 0;
  o[2] = (loaded & kMaskR) != 0;
  o[3] = (loaded & kMaskB) != 0;
}

size_t workspace_bytes(int N) { return ((size_t)N * 3 * 4 + 255) / 256 * 256; }

bool in_range(double dot) { return std::isfinite(dot) && dot >= -1.0 && dot <= 3.0; }

}  // namespace
}  // namespace pr

extern "C" int pr_activity_tile_rows(void) { return pr::kTileRows; }
extern "C" int pr_activity_chunk_rows(void) { return pr::kChunkRows; }

extern "C" size_t pr_activity_workspace_bytes(int N) { return N < 0 ? 0 : pr::workspace_bytes(N); }

extern "C" int pr_activity_tracks(const pr_activity_params* params, const float* rotmat_dev, const int32_t* frame_no_dev,
                                  const int* track_start_host, int T, int N, int32_t* flags_dev, int32_t* adds_dev,
                                  void* workspace_dev, void* stream) {
  using namespace pr;
  PR_REQUIRE(params, "pr_activity_tracks: null params");
  const int H = params->hold_frames, R = params->rapid_frames, G = params->gap_frames, E = params->rep_events;
  PR_REQUIRE(H >= 1 && H <= kMaxHold, "pr_activity_tracks: hold_frames = %d outside 1..%d", H, kMaxHold);
  PR_REQUIRE(R >= 1 && R <= H, "pr_activity_tracks: rapid_frames = %d outside 1..hold_frames = %d", R, H);
  PR_REQUIRE(G >= 1, "pr_activity_tracks: gap_frames = %d, not >= 1", G);
  PR_REQUIRE(E >= 0, "pr_activity_tracks: rep_events = %d, not >= 0", E);
  PR_REQUIRE(in_range(params->dot_static), "pr_activity_tracks: dot_static = %g is not a finite number in [-1, 3]", params->dot_static);
  PR_REQUIRE(in_range(params->dot_move), "pr_activity_tracks: dot_move = %g is not a finite number in [-1, 3]", params->dot_move);
  PR_REQUIRE(in_range(params->dot_rapid), "pr_activity_tracks: dot_rapid = %g is not a finite number in [-1, 3]", params->dot_rapid);
  PR_REQUIRE(N >= 0 && N <= kMaxRows, "pr_activity_tracks: N = %d outside 0..%d", N, kMaxRows);
  PR_REQUIRE(T >= 0, "pr_activity_tracks: T = %d", T);
  PR_REQUIRE(track_start_host, "pr_activity_tracks: null track_start");
  PR_REQUIRE(track_start_host[0] == 0, "pr_activity_tracks: track_start[0] = %d, not 0", track_start_host[0]);
  for (int t = 0; t < T; ++t)
    PR_REQUIRE(track_start_host[t] <= track_start_host[t + 1], "pr_activity_tracks: track_start[%d] = %d > track_start[%d] = %d", t,
               track_start_host[t], t + 1, track_start_host[t + 1]);
  PR_REQUIRE(track_start_host[T] == N, "pr_activity_tracks: track_start[T = %d] = %d, not N = %d", T, track_start_host[T], N);
  if (N == 0) return PR_OK;
  PR_REQUIRE(rotmat_dev && frame_no_dev, "pr_activity_tracks: null rotmat or frame_no");
  PR_REQUIRE(flags_dev && adds_dev, "pr_activity_tracks: null flags or adds");
  PR_REQUIRE(workspace_dev, "pr_activity_tracks: null workspace");
  PR_REQUIRE((uintptr_t)workspace_dev % 4 == 0, "pr_activity_tracks: workspace not 4-byte aligned");
  {
    const void* all[] = {rotmat_dev, frame_no_dev, flags_dev, adds_dev, workspace_dev};
    for (size_t x = 0; x < sizeof all / sizeof all[0]; ++x)
      for (size_t y = 0; y < x; ++y) PR_REQUIRE(all[x] != all[y], "pr_activity_tracks: two arguments share one pointer");
  }
  int32_t* ws = (int32_t*)workspace_dev;
  hipStream_t s = (hipStream_t)stream;
  for (int t0 = 0; t0 < T; t0 += kMaxTracks) {
    const int t1 = std::min(t0 + kMaxTracks, T);
    Params p{};
    p.rotmat = rotmat_dev;
    p.frame_no = frame_no_dev;
    p.moved = ws;
    p.held_rep = ws + N;
    p.rapid = ws + 2 * (size_t)N;
    p.flags = flags_dev;
    p.adds = adds_dev;
    p.dot_static = params->dot_static;
    p.dot_move = params->dot_move;
    p.dot_rapid = params->dot_rapid;
    p.H = H;
    p.R = R;
    p.G = G;
    p.E = E;
    p.row0 = track_start_host[t0];
    p.row1 = track_start_host[t1];
    p.n_tracks = t1 - t0;
    if (p.row1 == p.row0) continue;
    for (int t = t0; t <= t1; ++t) p.start[t - t0] = track_start_host[t];
    const int rows = p.row1 - p.row0;
    hipLaunchKernelGGL(events_kernel, dim3((unsigned)p.n_tracks), dim3(kThreads), 0, s, p);
    PR_TRY(check_launch("events_kernel"));
    hipLaunchKernelGGL(window_kernel, dim3((unsigned)ceil_div(rows, kTileRows)), dim3(kWindowThreads), 0, s, p);
    PR_TRY(check_launch("window_kernel"));
    hipLaunchKernelGGL(spread_kernel, dim3((unsigned)ceil_div(rows, kThreads)), dim3(kThreads), 0, s, p);
    PR_TRY(check_launch("spread_kernel"));
  }
  return PR_OK;
}
