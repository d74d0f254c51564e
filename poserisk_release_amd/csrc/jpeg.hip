// Device half of the JPEG decoder: everything behind the marker parser of csrc/jpeg_host.cc.  The contract -- the arithmetic,
// the 32-bit IDCT bound, what a bad stream may and may not do -- is written in include/poserisk_hip.h above pr_jpeg_parse;
// tests/jpeg_ref.py restates it in numpy, tests/test_jpeg_native.py runs this file on the host under sanitizers and
// tests/test_jpeg_gpu.py compares every byte with libjpeg's.
//
//   entropy  one LANE per restart segment (the whole scan where a frame has none), the lanes spread over as many waves as the
//            machine holds (kEntropyWavesPerCu below): Huffman decode (9-bit look-ahead table,
//            then length by length), receive-and-extend, DC prediction, zig-zag -> natural order.  Only NON-ZERO coefficients
//            are written, as int16, over a workspace the entry point has cleared.  A frame without restart markers is one
//            serial chain on one lane: the kernel's rate comes from the number of frames (segments) per call.  The decode
//            tables stay in global memory (5.6 KB a set, read-only, shared by every frame one encoder wrote: L2 / the vector
//            L1 hold them); each lane walks its own stream, four file bytes a load where none of them is 0xFF.
//   idct     one lane per 8x8 block: dequantise, islow IDCT in 32-bit (exactness bound checked per block), range limit, eight
//            8-byte stores into the component's block-padded u8 plane.
//   colour   one lane per four output pixels (twelve bytes, three aligned dword stores): fancy chroma upsampling from the
//            planes, YCbCr -> RGB, crop to H x W.
// Kernels index by thread only: no LDS, no barrier, no cross-lane operation, plain C++ and vector stores.
#include "common.h"
#include "jpeg_device.h"

namespace pr {
namespace {

constexpr int kEntropyThreads = 64;   // one wave a workgroup
// Segments are dealt to waves as thinly as the machine allows: `lanes` of a wave's 64 work, the fewest that still fit every
// segment into kEntropyWavesPerCu waves a CU.  A lane's loop is a chain of dependent loads whose time does not depend on how many
// lanes share its wave, while every data-dependent branch (refill, long code, end of block, run of sixteen) is paid once per
// path taken in the wave: a batch of 64 restart-free frames runs as 64 waves of one lane on 64 CUs, not as one divergent wave.
// Measured against 1 and 4 waves a CU in DESIGN.md section 3.9 (ablation builds: POSERISK_CXXFLAGS=-DPR_JPEG_ENTROPY_WAVES_PER_CU=n).
#ifndef PR_JPEG_ENTROPY_WAVES_PER_CU
#define PR_JPEG_ENTROPY_WAVES_PER_CU 16
#endif
constexpr int kEntropyWavesPerCu = PR_JPEG_ENTROPY_WAVES_PER_CU;
constexpr int kThreads = 256;

__global__ void __launch_bounds__(kEntropyThreads) jpeg_entropy_kernel(JpegParams p) {
  const pr_jpeg_args& a = p.a;
  const int t = (int)blockIdx.x * p.lanes + (int)threadIdx.x;
  if ((int)threadIdx.x >= p.lanes || t >= a.n_segments) return;
  const pr_jpeg_segment sg = a.segments[t];
  if ((unsigned)sg.frame >= (unsigned)a.F) return;               // belongs to no frame of this call
  const pr_jpeg_frame& fr = a.frames[sg.frame];
  if (!frame_ok(fr, a)) return;                                   // the colour kernel reports it
  if (p.gate && !p.gate[sg.frame].fell_back) return;             // pr_jpeg_decode_sync: the sub-sequence kernels decoded it
  const Geometry g = geometry(fr);
  const int total = g.mx * g.my;
  if (sg.begin < 0 || sg.end > a.data_bytes || sg.begin > sg.end || sg.first_mcu < 0 || sg.first_mcu >= total) {
    atomicOr(a.status + sg.frame, (int)PR_JPEG_ST_REFUSED);
    return;
  }
  const int n_mcus = fr.restart_interval > 0 ? min(fr.restart_interval, total - sg.first_mcu) : total - sg.first_mcu;
  const pr_jpeg_huff& tabs = a.huff[fr.huff_set];
  const int ncomp = fr.ncomp, fhs = fr.hs, fvs = fr.vs;   // locals: the stores below must not make the loop reload them
  const pr_jpeg_hufftab* dct[3];
  const pr_jpeg_hufftab* act[3];
  for (int c = 0; c < 3; ++c) {
    dct[c] = &tabs.tab[fr.dc_sel[c]];
    act[c] = &tabs.tab[2 + fr.ac_sel[c]];
  }
  short* coef = p.coef + (long)sg.frame * p.cs;
  Bits b;
  b.data = a.data;
  b.pos = sg.begin;
  b.end = sg.end;
  b.acc = 0ull;
  b.cnt = 0;
  b.pad = 0;
  b.ended = false;
  b.st = 0;
  b.marks = 0u;
  int pred[3] = {0, 0, 0};
  int mxi = sg.first_mcu % g.mx, myi = sg.first_mcu / g.mx;
  bool dead = false;
  for (int m = 0; m < n_mcus && !dead; ++m) {
    for (int c = 0; c < ncomp && !dead; ++c) {
      const int hc = c == 0 ? fhs : 1, vc = c == 0 ? fvs : 1;
      const pr_jpeg_hufftab& dc = *dct[c];
      const pr_jpeg_hufftab& ac = *act[c];
      for (int blk = 0; blk < hc * vc && !dead; ++blk) {
        const int bx = mxi * hc + (blk % hc), by = myi * vc + (blk / hc);
        short* out = coef + g.off[c] + ((long)by * g.bw[c] + bx) * 64;
        int s = next_symbol(b, dc);
        if (s < 0 || s > 15) {
          b.st |= PR_JPEG_ST_BAD_CODE;
          dead = true;
          break;
        }
        if (s) pred[c] += receive_extend(b, s);
        if (pred[c] != (short)pred[c]) {   // flagged and held at the int16 limit: the sum never leaves int however long it runs
          b.st |= PR_JPEG_ST_COEF_RANGE;
          pred[c] = pred[c] < 0 ? -32768 : 32767;
        }
        if (pred[c]) out[0] = (short)pred[c];
        for (int k = 1; k < 64;) {
          const int rs = next_symbol(b, ac);
          if (rs < 0) {
            b.st |= PR_JPEG_ST_BAD_CODE;
            dead = true;
            break;
          }
          const int r = rs >> 4;
          s = rs & 15;
          if (s == 0) {
            if (r != 15) break;                                   // end of block
            k += 16;
            if (k > 63) {                                         // sixteen zeros with no coefficient left behind them
              b.st |= PR_JPEG_ST_BAD_RUN;
              break;
            }
            continue;
          }
          k += r;
          if (k > 63) {
            b.st |= PR_JPEG_ST_BAD_RUN;
            break;
          }
          const int v = receive_extend(b, s);
          out[kZigzagNatural[k]] = (short)v;
          ++k;
        }
      }
    }
    if (++mxi == g.mx) {
      mxi = 0;
      ++myi;
    }
  }
  if (b.st) atomicOr(a.status + sg.frame, b.st);
}

// ---- dequantisation + islow IDCT ------------------------------------------------------------------------------------------
// One 1-D pass in 32-bit two's complement (unsigned, so that wrapping is defined): the values BEFORE the descale.
__device__ __forceinline__ void idct_pass(const int* in, int stride, unsigned* o) {
  const unsigned i0 = (unsigned)in[0], i1 = (unsigned)in[stride], i2 = (unsigned)in[2 * stride], i3 = (unsigned)in[3 * stride],
                 i4 = (unsigned)in[4 * stride], i5 = (unsigned)in[5 * stride], i6 = (unsigned)in[6 * stride],
                 i7 = (unsigned)in[7 * stride];
  unsigned z1 = (i2 + i6) * 4433u;
  const unsigned t2 = z1 - i6 * 15137u, t3 = z1 + i2 * 6270u;
  const unsigned t0 = (i0 + i4) << 13, t1 = (i0 - i4) << 13;
  const unsigned t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  unsigned a0 = i7, a1 = i5, a2 = i3, a3 = i1;
  z1 = a0 + a3;
  unsigned z2 = a1 + a2, z3 = a0 + a2, z4 = a1 + a3;
  const unsigned z5 = (z3 + z4) * 9633u;
  a0 *= 2446u;
  a1 *= 16819u;
  a2 *= 25172u;
  a3 *= 12299u;
  z1 *= (unsigned)-7373;
  z2 *= (unsigned)-20995;
  z3 = z3 * (unsigned)-16069 + z5;
  z4 = z4 * (unsigned)-3196 + z5;
  a0 += z1 + z3;
  a1 += z2 + z4;
  a2 += z2 + z3;
  a3 += z1 + z4;
  o[0] = t10 + a3;
  o[1] = t11 + a2;
  o[2] = t12 + a1;
  o[3] = t13 + a0;
  o[4] = t13 - a0;
  o[5] = t12 - a1;
  o[6] = t11 - a2;
  o[7] = t10 - a3;
}

__device__ __forceinline__ int descale(unsigned v, int n) { return (int)(v + (1u << (n - 1))) >> n; }

__device__ __forceinline__ bool beyond(int v) { return v > PR_JPEG_IDCT_BOUND || v < -PR_JPEG_IDCT_BOUND; }

__global__ void __launch_bounds__(kThreads) jpeg_idct_kernel(JpegParams p) {
  const pr_jpeg_args& a = p.a;
  const int f = (int)blockIdx.y;
  long b = (long)blockIdx.x * kThreads + (long)threadIdx.x;
  const pr_jpeg_frame& fr = a.frames[f];
  if (!frame_ok(fr, a)) return;
  const Geometry g = geometry(fr);
  int c = 0;
  for (; c < fr.ncomp; ++c) {
    const long n = (long)g.bw[c] * g.bh[c];
    if (b < n) break;
    b -= n;
  }
  if (c == fr.ncomp) return;
  const int by = (int)(b / g.bw[c]), bx = (int)(b - (long)by * g.bw[c]);
  short q[64];
  unsigned short qt[64];
  __builtin_memcpy(q, p.coef + (long)f * p.cs + g.off[c] + b * 64, 128);
  __builtin_memcpy(qt, fr.quant[c], 128);
  int d[64], w[64];
  bool far = false;
#pragma unroll
  for (int k = 0; k < 64; ++k) {
    d[k] = (int)q[k] * (int)qt[k];          // |.| <= 32768 * 65535 < 2^31
    far = far || beyond(d[k]);
  }
#pragma unroll
  for (int col = 0; col < 8; ++col) {
    unsigned o[8];
    idct_pass(d + col, 8, o);
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      w[8 * r + col] = descale(o[r], 11);
      far = far || beyond(w[8 * r + col]);
    }
  }
  unsigned char* plane = p.planes + (long)f * p.cs + g.off[c];
  const int pitch = g.bw[c] * 8;
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    unsigned o[8];
    idct_pass(w + 8 * r, 1, o);
    unsigned char px[8];
#pragma unroll
    for (int col = 0; col < 8; ++col) {
      const int x = (descale(o[col], 18) + 128) & 1023;   // libjpeg's range-limit table with its wrap
      px[col] = (unsigned char)(x < 256 ? x : (x < 512 ? 255 : 0));
    }
    __builtin_memcpy(plane + ((long)by * 8 + r) * pitch + bx * 8, px, 8);
  }
  if (far) atomicOr(a.status + f, (int)PR_JPEG_ST_IDCT_RANGE);
}

// ---- chroma upsampling + colour conversion --------------------------------------------------------------------------------
// One chroma sample at full resolution (x, y) from the component's plane s (pitch in samples), its own size dw x dh.
__device__ __forceinline__ int upsample(const unsigned char* s, int pitch, int dw, int dh, int hs, int vs, int x, int y) {
  if (hs == 1) return s[(long)y * pitch + x];
  const int i = x >> 1;
  if (vs == 1) {
    const unsigned char* row = s + (long)y * pitch;
    if (x & 1) return i == dw - 1 ? row[i] : (3 * row[i] + row[i + 1] + 2) >> 2;
    return i == 0 ? row[0] : (3 * row[i] + row[i - 1] + 1) >> 2;
  }
  const int r = y >> 1;
  const int r2 = (y & 1) ? min(r + 1, dh - 1) : max(r - 1, 0);
  const unsigned char* near = s + (long)r * pitch;
  const unsigned char* other = s + (long)r2 * pitch;
  const int ci = 3 * near[i] + other[i];
  if (x & 1) return i == dw - 1 ? (4 * ci + 7) >> 4 : (3 * ci + 3 * near[i + 1] + other[i + 1] + 7) >> 4;
  return i == 0 ? (4 * ci + 8) >> 4 : (3 * ci + 3 * near[i - 1] + other[i - 1] + 8) >> 4;
}

__device__ __forceinline__ int clamp255(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

__global__ void __launch_bounds__(kThreads) jpeg_colour_kernel(JpegParams p) {
  const pr_jpeg_args& a = p.a;
  const long hw = (long)a.H * a.W, total = hw * a.F;
  const long px0 = ((long)blockIdx.x * kThreads + (long)threadIdx.x) * 4;
  if (px0 >= total) return;
  int f = (int)(px0 / hw);
  const long rem = px0 - (long)f * hw;
  int y = (int)(rem / a.W), x = (int)(rem - (long)y * a.W);
  int loaded = -1;
  bool ok = false;
  Geometry g = {};
  int ncomp = 0, hs = 1, vs = 1, dw = 0, dh = 0;
  const unsigned char* plane = nullptr;
  unsigned char bytes[12];
  const int npx = (int)min(4l, total - px0);
  for (int q = 0; q < 4; ++q) {
    int R = 0, G = 0, B = 0;
    if (q < npx) {
      if (f != loaded) {
        const pr_jpeg_frame& fr = a.frames[f];
        ok = frame_ok(fr, a);
        if (ok) {
          g = geometry(fr);
          ncomp = fr.ncomp;
          hs = fr.hs;
          vs = fr.vs;
          dw = (a.W + hs - 1) / hs;
          dh = (a.H + vs - 1) / vs;
          plane = p.planes + (long)f * p.cs;
        }
        loaded = f;
      }
      if (!ok) {
        if (x == 0 && y == 0) atomicOr(a.status + f, (int)PR_JPEG_ST_REFUSED);
      } else {
        const int Y = plane[(long)y * (g.bw[0] * 8) + x];
        if (ncomp == 1) {
          R = G = B = Y;
        } else {
          const int cb = upsample(plane + g.off[1], g.bw[1] * 8, dw, dh, hs, vs, x, y) - 128;
          const int cr = upsample(plane + g.off[2], g.bw[2] * 8, dw, dh, hs, vs, x, y) - 128;
          R = clamp255(Y + ((91881 * cr + 32768) >> 16));
          G = clamp255(Y + ((-22554 * cb + 32768 - 46802 * cr) >> 16));
          B = clamp255(Y + ((116130 * cb + 32768) >> 16));
        }
      }
      if (++x == a.W) {
        x = 0;
        if (++y == a.H) {
          y = 0;
          ++f;
        }
      }
    }
    bytes[3 * q] = (unsigned char)(a.bgr ? B : R);
    bytes[3 * q + 1] = (unsigned char)G;
    bytes[3 * q + 2] = (unsigned char)(a.bgr ? R : B);
  }
  unsigned char* dst = a.out + px0 * 3;
  if (npx == 4 && p.out_aligned) {
    __builtin_memcpy(__builtin_assume_aligned(dst, 4), bytes, 12);   // three dword stores: 3 px0 is a multiple of 12
  } else {
    for (int i = 0; i < 3 * npx; ++i) dst[i] = bytes[i];
  }
}

}  // namespace

int jpeg_launch_serial_entropy(const JpegParams& params, hipStream_t s) {
  if (params.a.n_segments <= 0) return PR_OK;
  JpegParams p = params;
  int cus = 0;
  PR_TRY(current_device_cus(&cus));
  p.lanes = std::min(kEntropyThreads, std::max(1, ceil_div(p.a.n_segments, cus * kEntropyWavesPerCu)));
  hipLaunchKernelGGL(jpeg_entropy_kernel, dim3((unsigned)ceil_div(p.a.n_segments, p.lanes)), dim3(kEntropyThreads), 0, s, p);
  return check_launch("jpeg_entropy_kernel");
}

int jpeg_launch_back_end(const JpegParams& p, hipStream_t s) {
  const long quads = ceil_div((long)p.a.F * p.a.H * p.a.W, 4l);
  hipLaunchKernelGGL(jpeg_idct_kernel, dim3((unsigned)ceil_div(p.cs / 64, (long)kThreads), (unsigned)p.a.F), dim3(kThreads), 0, s, p);
  PR_TRY(check_launch("jpeg_idct_kernel"));
  hipLaunchKernelGGL(jpeg_colour_kernel, dim3((unsigned)ceil_div(quads, (long)kThreads)), dim3(kThreads), 0, s, p);
  return check_launch("jpeg_colour_kernel");
}
}  // namespace pr

extern "C" size_t pr_jpeg_workspace_bytes(int F, int H, int W) {
  if (F <= 0 || H <= 0 || W <= 0 || H > 4096 || W > 4096) return 0;
  return (size_t)F * (size_t)pr::padded_samples(H, W) * 3u;   // int16 coefficients + u8 planes
}

extern "C" int pr_jpeg_decode(const pr_jpeg_args* a, void* workspace, size_t workspace_bytes, void* stream) {
  using namespace pr;
  PR_REQUIRE(a, "pr_jpeg_decode: null argument struct");
  PR_REQUIRE(a->F >= 0, "pr_jpeg_decode: F = %d", a->F);
  if (a->F == 0) return PR_OK;
  PR_REQUIRE(a->F <= 65535, "pr_jpeg_decode: F = %d frames in one call (at most 65535)", a->F);
  PR_REQUIRE(a->H >= 16 && a->W >= 16 && a->H <= 4096 && a->W <= 4096, "pr_jpeg_decode: H x W = %d x %d outside 16..4096", a->H,
             a->W);
  PR_REQUIRE(a->frames, "pr_jpeg_decode: null frames");
  PR_REQUIRE(a->out, "pr_jpeg_decode: null out");
  PR_REQUIRE(a->status, "pr_jpeg_decode: null status");
  PR_REQUIRE(a->n_segments >= 0 && a->n_huff >= 0 && a->data_bytes >= 0,
             "pr_jpeg_decode: negative count (n_segments %d, n_huff %d, data_bytes %lld)", a->n_segments, a->n_huff,
             (long long)a->data_bytes);
  PR_REQUIRE(a->n_segments == 0 || (a->segments && a->data && a->huff && a->n_huff > 0 && a->data_bytes > 0),
             "pr_jpeg_decode: %d segments need data, segments and huff (null pointer, n_huff = %d or data_bytes = %lld)",
             a->n_segments, a->n_huff, (long long)a->data_bytes);
  PR_REQUIRE(workspace, "pr_jpeg_decode: null workspace");
  PR_REQUIRE(((uintptr_t)workspace & 15) == 0, "pr_jpeg_decode: workspace is not 16-byte aligned");
  const size_t need = pr_jpeg_workspace_bytes(a->F, a->H, a->W);
  PR_REQUIRE(workspace_bytes >= need, "pr_jpeg_decode: workspace of %zu bytes, %zu needed for %d frames of %d x %d",
             workspace_bytes, need, a->F, a->H, a->W);
  const long quads = ceil_div((long)a->F * a->H * a->W, 4l);
  PR_REQUIRE(quads <= (1l << 38), "pr_jpeg_decode: %d frames of %d x %d are too many pixels for one call", a->F, a->H, a->W);
  JpegParams p;
  p.a = *a;
  p.cs = padded_samples(a->H, a->W);
  p.out_aligned = ((uintptr_t)a->out & 3) == 0;
  p.lanes = 1;
  p.gate = nullptr;
  p.coef = (short*)workspace;
  p.planes = (unsigned char*)workspace + (size_t)a->F * p.cs * 2;
  hipStream_t s = (hipStream_t)stream;
  PR_HIP(hipMemsetAsync(p.coef, 0, (size_t)a->F * p.cs * 2, s));
  PR_HIP(hipMemsetAsync(a->status, 0, (size_t)a->F * sizeof(int32_t), s));
  PR_TRY(jpeg_launch_serial_entropy(p, s));
  return jpeg_launch_back_end(p, s);
}
