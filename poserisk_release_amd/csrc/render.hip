// Mesh overlay (ABI 12): the fitted SMPL mesh of every crop rasterised over its video frame, flat shaded, one colour per body
// part.  The raster contract -- projection, fixed point, coverage, visibility, shading -- is written in include/poserisk_hip.h
// above pr_render_overlay; tests/raster_ref.py restates it in numpy and tests/test_render_gpu.py compares face_id bit for bit.
//
// One rasteriser, two entries.  pr_render_people (header section r4) draws N meshes on M canvases with one key buffer
// u64[M,H,W], so that the people of a frame are depth-tested against each other; pr_render_overlay is its identity case, one
// mesh per canvas: M = N, mesh n on canvas n over frame frame_idx[n], no depth step (People below, `canvas == nullptr`).
//
// Five launches on the caller's stream, no allocation, no synchronisation:
//   clear     key buffer := ~0, the big-face queue's counter := 0, status[n] and canvas_status[m] := their index bits
//   vertex    one thread per (mesh, vertex): projection -> int32x4 (xf, yf, zf, valid)
//   face      one thread per (mesh, face): setup, clipped box, packed colour; boxes of <= kSmallBox pixels rasterised in the
//             thread with 64-bit atomicMin on the key, larger ones appended to a queue
//   big face  a grid-stride loop of workgroups over the queue, threads over the face's box
//   resolve   one thread per output pixel: key -> face colour, blend with the frame, write out (and face_id)
// A key's low half is n F + f, which is also the face's slot in the colour table and in the big-face queue.  The smallest key
// wins whatever the order of the atomics, so the result is bit-for-bit deterministic.
#include "common.h"

namespace pr {
namespace {

constexpr int kSmallBox = 64;        // box pixels a face thread rasterises itself
constexpr int kBigThreads = 256;     // threads per queued face
constexpr int kBigBlocks = 2048;     // workgroups of the big-face pass (grid-stride over the queue)
constexpr double kFix = 16.0;        // sub-pixel steps per pixel
constexpr double kZFix = 4096.0;     // depth steps per metre
constexpr int kZBias = 1 << 20;      // keeps zf positive for |Z| < 256 m
constexpr double kGuard = 4096.0;    // a vertex this far outside the frame is invalid
constexpr double kZMax = 256.0;

struct Geo {
  const float* verts;
  const int32_t* faces;
  const float* cam;
  const float* bboxes;
  int N, V, F, H, W, n_frames;
  float scale;
};

// Where the meshes go.  canvas == nullptr is pr_render_overlay's identity case (internal: pr_render_people refuses a null
// canvas when it has meshes): mesh n on canvas n, M = N, no depth step -- neither canvas[n] nor z_step[n] is loaded.
struct People {
  const int32_t* canvas;
  const int32_t* src_idx;   // the source frame of canvas m (pr_render_overlay: frame_idx); nullptr: frame m
  const int32_t* z_step;
  int M;
};

constexpr int kZStepMax = PR_RENDER_Z_STEP_MAX;

__device__ __forceinline__ long long orient2d(int ax, int ay, int bx, int by, int cx, int cy) {
  return (long long)(bx - ax) * (long long)(cy - ay) - (long long)(by - ay) * (long long)(cx - ax);
}

// a pixel sample on an edge (weight 0) belongs to the face iff the edge P->Q has dy > 0, or dy == 0 and dx < 0
__device__ __forceinline__ bool owns_edge(int dx, int dy) { return dy > 0 || (dy == 0 && dx < 0); }

// A face after setup: vertices in fixed point (b, c swapped when the projected winding is negative), doubled area A > 0 and
// the frame-clipped box.  false: nothing to draw (bad index, invalid vertex, zero area, box off the frame).
struct Setup {
  int ax, ay, az, bx, by, bz, cx, cy, cz;
  long long area;
  int x0, x1, y0, y1;
};

__device__ __forceinline__ bool face_setup(const Geo& g, const int4* __restrict__ vfx, int n, int f, Setup& s, bool* bad_index) {
  const int ia = g.faces[3 * f], ib = g.faces[3 * f + 1], ic = g.faces[3 * f + 2];
  *bad_index = (unsigned)ia >= (unsigned)g.V || (unsigned)ib >= (unsigned)g.V || (unsigned)ic >= (unsigned)g.V;
  if (*bad_index) return false;
  const long base = (long)n * g.V;
  int4 a = vfx[base + ia], b = vfx[base + ib], c = vfx[base + ic];
  if (!a.w || !b.w || !c.w) return false;
  long long area = orient2d(a.x, a.y, b.x, b.y, c.x, c.y);
  if (area == 0) return false;
  if (area < 0) {
    const int4 t = b;
    b = c;
    c = t;
    area = -area;
  }
  s.ax = a.x; s.ay = a.y; s.az = a.z;
  s.bx = b.x; s.by = b.y; s.bz = b.z;
  s.cx = c.x; s.cy = c.y; s.cz = c.z;
  s.area = area;
  // samples at 16 j: j from ceil(min / 16) to floor(max / 16) (arithmetic shifts floor negative values)
  const int xmin = min(a.x, min(b.x, c.x)), xmax = max(a.x, max(b.x, c.x));
  const int ymin = min(a.y, min(b.y, c.y)), ymax = max(a.y, max(b.y, c.y));
  s.x0 = max((xmin + 15) >> 4, 0);
  s.x1 = min(xmax >> 4, g.W - 1);
  s.y0 = max((ymin + 15) >> 4, 0);
  s.y1 = min(ymax >> 4, g.H - 1);
  return s.x0 <= s.x1 && s.y0 <= s.y1;
}

// Coverage and depth of sample (16 j, 16 i); returns the key, or ~0 when the sample is not covered.
__device__ __forceinline__ unsigned long long sample_key(const Setup& s, int j, int i, unsigned f) {
  const int px = 16 * j, py = 16 * i;
  const long long w0 = orient2d(s.bx, s.by, s.cx, s.cy, px, py);
  const long long w1 = orient2d(s.cx, s.cy, s.ax, s.ay, px, py);
  const long long w2 = orient2d(s.ax, s.ay, s.bx, s.by, px, py);
  const bool in0 = w0 > 0 || (w0 == 0 && owns_edge(s.cx - s.bx, s.cy - s.by));
  const bool in1 = w1 > 0 || (w1 == 0 && owns_edge(s.ax - s.cx, s.ay - s.cy));
  const bool in2 = w2 > 0 || (w2 == 0 && owns_edge(s.bx - s.ax, s.by - s.ay));
  if (!(in0 && in1 && in2)) return ~0ull;
  // every term is non-negative, so truncation is floor
  const long long depth = (w0 * s.az + w1 * s.bz + w2 * s.cz) / s.area;
  return ((unsigned long long)depth << 32) | f;
}

// Vertex i = n V + v of mesh n in fixed point (xf, yf, zf + z_step, 1); all zero when it is invalid.
__device__ __forceinline__ int4 project_vertex(const Geo& g, long i, int n, int z_step) {
  const float* p = g.verts + i * 3;
  const float* cm = g.cam + (long)n * 3;
  const float* bb = g.bboxes + (long)n * 4;
  const double X = p[0], Y = p[1], Z = p[2];
  const double s = cm[0], tx = cm[1], ty = cm[2];
  const double x = (double)bb[0] + s * (X + tx) * (double)bb[2] * (double)g.scale * 0.5;
  const double y = (double)bb[1] + s * (Y + ty) * (double)bb[3] * (double)g.scale * 0.5;
  const bool valid = isfinite(x) && isfinite(y) && isfinite(Z) && x > -kGuard && x < (g.W - 1) + kGuard && y > -kGuard &&
                     y < (g.H - 1) + kGuard && fabs(Z) < kZMax;
  if (!valid) return make_int4(0, 0, 0, 0);
  return make_int4(__double2int_rn(kFix * x), __double2int_rn(kFix * y), __double2int_rn(kZFix * Z) + kZBias + z_step, 1);
}

// Flat shading of face f of mesh n from the float vertices in the face's own order; the light is along the view axis,
// two-sided.  Returns the colour packed in quarter steps, 10 bits a channel.
__device__ __forceinline__ unsigned face_colour(const Geo& g, int n, int f, const int32_t* __restrict__ face_part,
                                                const uint8_t* __restrict__ part_rgb, int P, int bgr) {
  const long base = (long)n * g.V;
  const float* va = g.verts + (base + g.faces[3 * f]) * 3;
  const float* vb = g.verts + (base + g.faces[3 * f + 1]) * 3;
  const float* vc = g.verts + (base + g.faces[3 * f + 2]) * 3;
  const float e1x = vb[0] - va[0], e1y = vb[1] - va[1], e1z = vb[2] - va[2];
  const float e2x = vc[0] - va[0], e2y = vc[1] - va[1], e2z = vc[2] - va[2];
  const float nx = e1y * e2z - e1z * e2y, ny = e1z * e2x - e1x * e2z, nz = e1x * e2y - e1y * e2x;
  const float len = sqrtf(nx * nx + ny * ny + nz * nz);
  const float inten = 0.35f + 0.65f * (len > 0.f ? fabsf(nz) / len : 0.f);
  const int part = min(max(face_part[f], 0), P - 1);
  const uint8_t* rgb = part_rgb + ((long)n * P + part) * 3;
  unsigned packed = 0;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    // channel k of the frame's order, in quarter steps (10 bits: 4 * 255 = 1020)
    const float c = (float)rgb[bgr ? 2 - k : k] * inten;
    const unsigned q = (unsigned)min(__float2int_rn(4.f * c), 1020);
    packed |= q << (10 * k);
  }
  return packed;
}

// out = rint((1 - alpha) frame + alpha colour), clamped, for one pixel
__device__ __forceinline__ void blend_pixel(const uint8_t* __restrict__ src, unsigned packed, float alpha, uint8_t* __restrict__ o) {
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float c = 0.25f * (float)((packed >> (10 * k)) & 1023u);
    const int v = __float2int_rn((1.f - alpha) * (float)src[k] + alpha * c);
    o[k] = (uint8_t)min(max(v, 0), 255);
  }
}

__device__ __forceinline__ bool canvas_frame(const Geo& g, const People& p, int m, int* fi) {
  const int f = p.src_idx ? p.src_idx[m] : m;
  *fi = f;
  return (unsigned)f < (unsigned)g.n_frames;
}

// status bits 3 and 4 of mesh n, all the vertex pass needs; *m is its canvas when bit 3 is clear, *z its depth step when bit 4
// is.  The identity test is a kernel-argument compare, uniform over the grid.
__device__ __forceinline__ int mesh_place(const People& p, int n, int* m, int* z) {
  *m = n;
  *z = 0;
  if (!p.canvas) return 0;
  *m = p.canvas[n];
  if (p.z_step) *z = p.z_step[n];
  return ((unsigned)*m >= (unsigned)p.M ? 8 : 0) | (*z < 0 || *z > kZStepMax ? 16 : 0);
}

// status bits 0, 3 and 4 of mesh n (0: it is drawn)
__device__ __forceinline__ int mesh_state(const Geo& g, const People& p, int n, int* m, int* z) {
  const int bits = mesh_place(p, n, m, z);
  int fi;
  return bits || canvas_frame(g, p, *m, &fi) ? bits : 1;
}

__global__ void people_clear_kernel(unsigned long long* __restrict__ zbuf, long n_keys, unsigned* __restrict__ queue_count,
                                    int32_t* __restrict__ status, int32_t* __restrict__ canvas_status, Geo g, People p) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n_keys) zbuf[i] = ~0ull;
  if (i == 0) *queue_count = 0u;
  if (status && i < g.N) {
    int m, z;
    status[i] = mesh_state(g, p, (int)i, &m, &z);
  }
  if (canvas_status && i < p.M) {
    int fi;
    canvas_status[i] = canvas_frame(g, p, (int)i, &fi) ? 0 : 1;
  }
}

__global__ void people_vertex_kernel(Geo g, People p, int4* __restrict__ vfx, int32_t* __restrict__ status) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)g.N * g.V) return;
  const int n = (int)(i / g.V);
  int m, zs;
  if (mesh_place(p, n, &m, &zs)) {   // draws nothing: no vertex of it is looked at
    vfx[i] = make_int4(0, 0, 0, 0);
    return;
  }
  const int4 o = project_vertex(g, i, n, zs);
  if (!o.w && status) atomicOr(status + n, 2);
  vfx[i] = o;
}

__global__ void people_face_kernel(Geo g, People p, const int4* __restrict__ vfx, const int32_t* __restrict__ face_part,
                                   const uint8_t* __restrict__ part_rgb, int P, int bgr, unsigned* __restrict__ colour,
                                   unsigned long long* __restrict__ zbuf, unsigned* __restrict__ queue_count,
                                   unsigned* __restrict__ queue, int32_t* __restrict__ status) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)g.N * g.F) return;
  const int n = (int)(i / g.F), f = (int)(i - (long)n * g.F);
  int m, zs;
  if (mesh_state(g, p, n, &m, &zs)) return;   // no canvas, no depth, or a canvas the resolve pass zero-fills
  Setup s;
  bool bad_index;
  if (!face_setup(g, vfx, n, f, s, &bad_index)) {
    if (bad_index && status) atomicOr(status + n, 4);
    return;
  }
  colour[i] = face_colour(g, n, f, face_part, part_rgb, P, bgr);
  if ((s.x1 - s.x0 + 1) * (s.y1 - s.y0 + 1) > kSmallBox) {
    queue[atomicAdd(queue_count, 1u)] = (unsigned)i;
    return;
  }
  unsigned long long* zb = zbuf + (long)m * g.H * g.W;
  for (int y = s.y0; y <= s.y1; ++y)
    for (int x = s.x0; x <= s.x1; ++x) {
      const unsigned long long key = sample_key(s, x, y, (unsigned)i);
      if (key != ~0ull) atomicMin(zb + (long)y * g.W + x, key);
    }
}

__global__ void __launch_bounds__(kBigThreads) people_bigface_kernel(Geo g, People p, const int4* __restrict__ vfx,
                                                                     unsigned long long* __restrict__ zbuf,
                                                                     const unsigned* __restrict__ queue_count,
                                                                     const unsigned* __restrict__ queue) {
  const unsigned count = *queue_count;
  for (unsigned q = blockIdx.x; q < count; q += gridDim.x) {
    const unsigned i = queue[q];
    const int n = (int)(i / (unsigned)g.F), f = (int)(i - (unsigned)n * (unsigned)g.F);
    Setup s;
    bool bad_index;
    if (!face_setup(g, vfx, n, f, s, &bad_index)) continue;   // never: the face pass queued it after the same setup
    const int bw = s.x1 - s.x0 + 1, bh = s.y1 - s.y0 + 1;
    unsigned long long* zb = zbuf + (long)(p.canvas ? p.canvas[n] : n) * g.H * g.W;   // in [0, M): the face pass checked it
    for (int k = threadIdx.x; k < bw * bh; k += kBigThreads) {
      const int y = s.y0 + k / bw, x = s.x0 + k % bw;
      const unsigned long long key = sample_key(s, x, y, i);
      if (key != ~0ull) atomicMin(zb + (long)y * g.W + x, key);
    }
  }
}

__global__ void people_resolve_kernel(Geo g, People p, const unsigned long long* __restrict__ zbuf,
                                      const unsigned* __restrict__ colour, const uint8_t* __restrict__ frames, float alpha,
                                      uint8_t* __restrict__ out, int32_t* __restrict__ face_id) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long hw = (long)g.H * g.W;
  if (i >= (long)p.M * hw) return;
  const int m = (int)(i / hw);
  const long pix = i - (long)m * hw;
  uint8_t* o = out + i * 3;
  int fi;
  if (!canvas_frame(g, p, m, &fi)) {
    o[0] = 0; o[1] = 0; o[2] = 0;
    if (face_id) face_id[i] = -1;
    return;
  }
  const uint8_t* src = frames + ((long)fi * hw + pix) * 3;
  const unsigned long long key = zbuf[i];
  if (key == ~0ull) {
    o[0] = src[0]; o[1] = src[1]; o[2] = src[2];
    if (face_id) face_id[i] = -1;
    return;
  }
  const unsigned id = (unsigned)(key & 0xffffffffull);   // n F + f
  blend_pixel(src, colour[id], alpha, o);
  if (face_id) face_id[i] = (int32_t)(p.canvas ? id : id - (unsigned)m * (unsigned)g.F);   // pr_render_overlay: the local face f
}

inline size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

struct Layout {
  size_t zbuf, vfx, colour, queue, total;
};

// n_canvases key planes (pr_render_overlay: one per crop), the rest sized by the N meshes
inline Layout layout(int N, int n_canvases, int V, int F, int H, int W) {
  Layout l;
  l.zbuf = 0;
  l.vfx = l.zbuf + align256((size_t)n_canvases * H * W * 8);
  l.colour = l.vfx + align256((size_t)N * V * 16);
  l.queue = l.colour + align256((size_t)N * F * 4);
  l.total = l.queue + align256(16 + (size_t)N * F * 4);   // counter, then at most N * F entries
  return l;
}

inline int blocks_for(long n, int t) { return (int)((n + t - 1) / t); }

// Both entries from here: the argument checks -- each entry's own conditions in its own order and wording, the shared ones in
// `who`'s name --, the workspace layout and the launches.  overlay: pr_render_overlay's block, a.canvas null, a.M = a.N > 0 and
// a.src_idx its frame_idx.
int render(const char* who, bool overlay, const pr_render_people_args& a, void* workspace, size_t workspace_bytes, void* stream) {
  const bool meshes_fit = (long)a.N * a.V < (1l << 31) && (long)a.N * a.F < (1l << 31);
  if (overlay)
    PR_REQUIRE(a.verts && a.faces && a.cam && a.bboxes && a.frames && a.face_part && a.part_rgb && a.out,
               "pr_render_overlay: null required pointer (verts, faces, cam, bboxes, frames, face_part, part_rgb, out)");
  else
    PR_REQUIRE(a.frames && a.out, "pr_render_people: null required pointer (frames, out)");
  PR_REQUIRE(workspace, "%s: null workspace", who);
  if (overlay)
    PR_REQUIRE(a.V >= 3 && a.F >= 1 && a.P >= 1 && a.n_frames >= 1, "pr_render_overlay: bad sizes V=%d F=%d P=%d frames=%d", a.V,
               a.F, a.P, a.n_frames);
  else
    PR_REQUIRE(a.n_frames >= 1, "pr_render_people: n_frames = %d", a.n_frames);
  PR_REQUIRE(a.H >= 1 && a.W >= 1 && a.H <= 4096 && a.W <= 4096, "%s: frame %d x %d outside 1..4096", who, a.H, a.W);
  if (overlay) {
    PR_REQUIRE(meshes_fit && (long)a.N * a.H * a.W < (1l << 40), "pr_render_overlay: batch too large (N=%d V=%d F=%d)", a.N, a.V,
               a.F);
    PR_REQUIRE(a.scale > 0.f && a.scale < 1e6f, "%s: bbox scale %g", who, (double)a.scale);
  } else {
    PR_REQUIRE((long)a.M * a.H * a.W < (1l << 40), "pr_render_people: batch too large (M=%d)", a.M);
  }
  PR_REQUIRE(a.alpha >= 0.f && a.alpha <= 1.f, "%s: alpha %g outside [0, 1]", who, (double)a.alpha);
  if (overlay)
    PR_REQUIRE(a.src_idx || a.N <= a.n_frames, "pr_render_overlay: %d crops for %d frames without a frame index", a.N, a.n_frames);
  else
    PR_REQUIRE(a.src_idx || a.M <= a.n_frames, "pr_render_people: %d canvases for %d frames without src_idx", a.M, a.n_frames);
  if (!overlay && a.N > 0) {
    PR_REQUIRE(a.verts && a.faces && a.cam && a.bboxes && a.canvas && a.face_part && a.part_rgb,
               "pr_render_people: null required pointer (verts, faces, cam, bboxes, canvas, face_part, part_rgb)");
    PR_REQUIRE(a.V >= 3 && a.F >= 1 && a.P >= 1, "pr_render_people: bad sizes V=%d F=%d P=%d", a.V, a.F, a.P);
    PR_REQUIRE(meshes_fit, "pr_render_people: batch too large (N=%d V=%d F=%d)", a.N, a.V, a.F);
    PR_REQUIRE(a.scale > 0.f && a.scale < 1e6f, "%s: bbox scale %g", who, (double)a.scale);
  }
  const int V = a.N ? a.V : 0, F = a.N ? a.F : 0;
  const Layout l = layout(a.N, a.M, V, F, a.H, a.W);
  PR_REQUIRE(workspace_bytes >= l.total, "%s: workspace of %zu bytes, %zu needed (%s)", who, workspace_bytes, l.total,
             overlay ? "pr_render_workspace_bytes" : "pr_render_people_workspace_bytes");
  hipStream_t s = (hipStream_t)stream;
  char* ws = (char*)workspace;
  auto* zbuf = (unsigned long long*)(ws + l.zbuf);
  auto* vfx = a.vert_fx ? (int4*)a.vert_fx : (int4*)(ws + l.vfx);
  auto* colour = (unsigned*)(ws + l.colour);
  auto* qcount = (unsigned*)(ws + l.queue);
  auto* queue = qcount + 4;
  Geo g{a.verts, a.faces, a.cam, a.bboxes, a.N, V, F, a.H, a.W, a.n_frames, a.scale};
  People p{a.canvas, a.src_idx, a.z_step, a.M};
  const long n_keys = (long)a.M * a.H * a.W;
  hipLaunchKernelGGL(people_clear_kernel, dim3(blocks_for(std::max(n_keys, (long)a.N), 256)), dim3(256), 0, s, zbuf, n_keys,
                     qcount, a.status, a.canvas_status, g, p);
  PR_TRY(check_launch("people_clear_kernel"));
  if (a.N > 0) {
    hipLaunchKernelGGL(people_vertex_kernel, dim3(blocks_for((long)a.N * V, 256)), dim3(256), 0, s, g, p, vfx, a.status);
    PR_TRY(check_launch("people_vertex_kernel"));
    hipLaunchKernelGGL(people_face_kernel, dim3(blocks_for((long)a.N * F, 256)), dim3(256), 0, s, g, p, (const int4*)vfx,
                       a.face_part, a.part_rgb, a.P, a.bgr, colour, zbuf, qcount, queue, a.status);
    PR_TRY(check_launch("people_face_kernel"));
    hipLaunchKernelGGL(people_bigface_kernel, dim3(kBigBlocks), dim3(kBigThreads), 0, s, g, p, (const int4*)vfx, zbuf,
                       (const unsigned*)qcount, (const unsigned*)queue);
    PR_TRY(check_launch("people_bigface_kernel"));
  }
  hipLaunchKernelGGL(people_resolve_kernel, dim3(blocks_for(n_keys, 256)), dim3(256), 0, s, g, p,
                     (const unsigned long long*)zbuf, (const unsigned*)colour, a.frames, a.alpha, a.out, a.face_id);
  return check_launch("people_resolve_kernel");
}

}  // namespace
}  // namespace pr

extern "C" {

size_t pr_render_workspace_bytes(int N, int V, int F, int H, int W) {
  if (N <= 0 || V <= 0 || F <= 0 || H <= 0 || W <= 0) return 0;
  return pr::layout(N, N, V, F, H, W).total;
}

int pr_render_overlay(const pr_render_args* a, void* workspace, size_t workspace_bytes, void* stream) {
  PR_REQUIRE(a, "pr_render_overlay: null argument struct");
  PR_REQUIRE(a->N >= 0, "pr_render_overlay: N = %d", a->N);
  if (a->N == 0) return PR_OK;
  const pr_render_people_args people{a->verts, a->faces, a->cam, a->bboxes, a->frames, /*canvas*/ nullptr, a->frame_idx,
                                     /*z_step*/ nullptr, a->face_part, a->part_rgb, a->out, a->face_id, a->vert_fx, a->status,
                                     /*canvas_status*/ nullptr, a->N, /*M*/ a->N, a->V, a->F, a->P, a->n_frames, a->H, a->W,
                                     a->bgr, a->scale, a->alpha};
  return pr::render("pr_render_overlay", true, people, workspace, workspace_bytes, stream);
}

size_t pr_render_people_workspace_bytes(int N, int M, int V, int F, int H, int W) {
  if (N < 0 || M <= 0 || H <= 0 || W <= 0 || (N > 0 && (V <= 0 || F <= 0))) return 0;
  return N ? pr::layout(N, M, V, F, H, W).total : pr::layout(0, M, 0, 0, H, W).total;
}

int pr_render_people(const pr_render_people_args* a, void* workspace, size_t workspace_bytes, void* stream) {
  PR_REQUIRE(a, "pr_render_people: null argument struct");
  PR_REQUIRE(a->N >= 0 && a->M >= 0, "pr_render_people: N = %d, M = %d", a->N, a->M);
  if (a->M == 0) return PR_OK;
  return pr::render("pr_render_people", false, *a, workspace, workspace_bytes, stream);
}

}  // extern "C"
