// The multi-scan entropy stage (include/poserisk_hip.h, section j1b): progressive JPEG (SOF2) and sequential files whose
// components come in several scans, decoded into the int16 coefficient workspace that csrc/jpeg.hip's IDCT and colour kernels
// read.  tests/jpeg_scans_ref.py restates it in Python, tests/test_jpeg_scans_native.py runs this file on the host under
// sanitizers, tests/test_jpeg_scans_gpu.py compares every byte with libjpeg's.
//
// A LANE is one (scan, restart segment); the lanes are dealt thinly over one-wave workgroups as in jpeg_entropy_kernel.  One
// launch per LEVEL: scans of one level write disjoint coefficients (the parser's rule), a scan reads only what earlier levels
// wrote.  Scans of one level do share 8x8 blocks -- libjpeg's script refines luma AC 1..63 and every DC in the same level -- so
// a lane stores single coefficients (2-byte stores) and never writes a block back as a whole.
//   sequential, DC first, AC first   write the non-zero values over the cleared workspace and read nothing back.
//   DC refine   ORs 1 << Al into coefficient 0 with an atomic whose result nobody waits for: the low half of the block's first
//               dword, no load, no round trip.
//   AC refine   visits every coefficient of its band in every block and must know which are non-zero.  The block's 128 bytes
//               are fetched ONCE (eight 16-byte loads issued back to back, one wait) one block AHEAD: the loads of block n + 1
//               are in flight while block n is decoded.  The copy is kept in a per-lane slice of LDS, in ZIG-ZAG order, so the
//               inner loop indexes it by k without a table lookup; LDS rather than registers because k is data dependent (a
//               register array indexed by a variable goes to scratch, which is memory again) -- 132 bytes a lane (a stride of
//               33 dwords: no bank shared by two lanes at the same k), 8.4 KB a workgroup, 19 workgroups a CU, above the 12
//               waves a CU the lanes are dealt for.  Changed coefficients go to LDS and, as 2-byte stores, to the workspace.
// Plain C++ and vector stores; no barrier, no cross-lane operation.
#include "common.h"
#include "jpeg_device.h"

namespace pr {
namespace {

constexpr int kScanThreads = 64;      // one wave a workgroup
constexpr int kScanWavesPerCu = 12;   // dealt as thinly as jpeg_entropy_kernel's, over what fits: 134 VGPRs, three waves a SIMD
constexpr int kSliceDwords = 33;      // a lane's block copy: 64 int16 and one dword of padding

constexpr unsigned char kZz[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                   41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                   30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

struct ScanParams {
  JpegParams p;
  const pr_jpeg_scan* scans;
  const int32_t* seg_scan;
  int n_scans, n_levels, level;
};

struct Block16 {
  unsigned v[4];
};

// Every field of a scan record that later forms an address, a loop bound or a shift, for a frame that passed frame_ok.
__device__ __forceinline__ bool scan_ok(const pr_jpeg_scan& sc, const pr_jpeg_frame& fr, const ScanParams& q) {
  if ((unsigned)sc.level >= (unsigned)q.n_levels) return false;
  if (sc.ncomp < 1 || sc.ncomp > fr.ncomp) return false;
  for (int i = 0; i < 3; ++i) {
    if ((unsigned)sc.dc_sel[i] > 1u || (unsigned)sc.ac_sel[i] > 1u) return false;
    if (i < sc.ncomp && ((unsigned)sc.comp[i] >= (unsigned)fr.ncomp || (i > 0 && sc.comp[i] <= sc.comp[i - 1]))) return false;
  }
  if (sc.ss < 0 || sc.ss > sc.se || sc.se > 63 || (unsigned)sc.ah > 13u || (unsigned)sc.al > 13u) return false;
  if (sc.ss == 0 && sc.se != 0 && !(sc.se == 63 && sc.ah == 0 && sc.al == 0)) return false;   // DC alone, or sequential
  if (sc.ss > 0 && sc.ncomp != 1) return false;
  if ((unsigned)sc.huff_set >= (unsigned)q.p.a.n_huff || sc.restart_interval < 0) return false;
  return true;
}

__device__ __forceinline__ int get_bits(Bits& b, int n) {   // 1 <= n <= 14
  fill(b);
  const int v = (int)peek(b, n);
  consume(b, n);
  return v;
}

// v, or the int16 limit with PR_JPEG_ST_COEF_RANGE where it lies outside
__device__ __forceinline__ int in_int16(Bits& b, int v) {
  if (v == (short)v) return v;
  b.st |= PR_JPEG_ST_COEF_RANGE;
  return v < 0 ? -32768 : 32767;
}

// j1's block decode (csrc/jpeg.hip), statement for statement: a frame pr_jpeg_parse accepts gets pr_jpeg_decode's status.
__device__ __forceinline__ bool sequential_block(Bits& b, const pr_jpeg_hufftab& dc, const pr_jpeg_hufftab& ac, int& pred, short* out) {
  int s = next_symbol(b, dc);
  if (s < 0 || s > 15) {
    b.st |= PR_JPEG_ST_BAD_CODE;
    return false;
  }
  if (s) pred += receive_extend(b, s);
  if (pred != (short)pred) {
    b.st |= PR_JPEG_ST_COEF_RANGE;
    pred = pred < 0 ? -32768 : 32767;
  }
  if (pred) out[0] = (short)pred;
  for (int k = 1; k < 64;) {
    const int rs = next_symbol(b, ac);
    if (rs < 0) {
      b.st |= PR_JPEG_ST_BAD_CODE;
      return false;
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
    out[kZigzagNatural[k]] = (short)receive_extend(b, s);
    ++k;
  }
  return true;
}

__device__ __forceinline__ bool dc_first_block(Bits& b, const pr_jpeg_hufftab& dc, int al, int& pred, short* out) {
  const int s = next_symbol(b, dc);
  if (s < 0 || s > 15) {
    b.st |= PR_JPEG_ST_BAD_CODE;
    return false;
  }
  if (s) pred += receive_extend(b, s);
  if (pred != (short)pred) {   // held at the int16 limit: the sum never leaves int however long it runs
    b.st |= PR_JPEG_ST_COEF_RANGE;
    pred = pred < 0 ? -32768 : 32767;
  }
  const int v = in_int16(b, pred * (1 << al));
  if (v) out[0] = (short)v;
  return true;
}

// An EOBn symbol's run, this block included; false (PR_JPEG_ST_BAD_RUN) where it is longer than the `left` blocks of the segment.
__device__ __forceinline__ bool eob_run(Bits& b, int r, int left, int& eobrun) {
  eobrun = 1 << r;
  if (r) eobrun += get_bits(b, r);
  if (eobrun <= left) return true;
  b.st |= PR_JPEG_ST_BAD_RUN;
  return false;
}

__device__ __forceinline__ bool ac_first_block(Bits& b, const pr_jpeg_hufftab& ac, int ss, int se, int al, int left, int& eobrun,
                                               short* out) {
  if (eobrun > 0) {
    --eobrun;
    return true;
  }
  for (int k = ss; k <= se;) {
    const int rs = next_symbol(b, ac);
    if (rs < 0) {
      b.st |= PR_JPEG_ST_BAD_CODE;
      return false;
    }
    const int r = rs >> 4, s = rs & 15;
    if (s == 0 && r != 15) {
      if (!eob_run(b, r, left, eobrun)) return false;
      --eobrun;
      return true;
    }
    k += s ? r : 16;
    if (k > se) {   // a run that leaves the band (sixteen zeros with no coefficient left behind them included)
      b.st |= PR_JPEG_ST_BAD_RUN;
      return false;
    }
    if (s) {
      const int v = in_int16(b, receive_extend(b, s) * (1 << al));
      out[kZigzagNatural[k]] = (short)v;
      ++k;
    }
  }
  return true;
}

// A correction bit for the non-zero coefficient blk[k] (zig-zag order; `out` is the block in the workspace, natural order).
__device__ __forceinline__ void correct(Bits& b, short* blk, short* out, int k, int p1) {
  if (!get_bits(b, 1)) return;
  const int c = blk[k];
  if (c & p1) return;
  const int v = in_int16(b, c >= 0 ? c + p1 : c - p1);
  blk[k] = (short)v;
  out[kZigzagNatural[k]] = (short)v;
}

// T.81 G.1.2.3 as libjpeg's decode_mcu_AC_refine walks it.  blk: the lane's copy of the block, zig-zag order.
__device__ __forceinline__ bool ac_refine_block(Bits& b, const pr_jpeg_hufftab& ac, int ss, int se, int al, int left, int& eobrun,
                                                short* blk, short* out) {
  const int p1 = 1 << al;
  int k = ss;
  if (eobrun == 0) {
    while (k <= se) {
      const int rs = next_symbol(b, ac);
      if (rs < 0) {
        b.st |= PR_JPEG_ST_BAD_CODE;
        return false;
      }
      int r = rs >> 4;
      const int s = rs & 15;
      int val = 0;
      if (s) {
        if (s != 1) {   // a new coefficient is +-1 at this bit position
          b.st |= PR_JPEG_ST_BAD_CODE;
          return false;
        }
        val = get_bits(b, 1) ? p1 : -p1;
      } else if (r != 15) {
        if (!eob_run(b, r, left, eobrun)) return false;
        break;
      }
      // pass r zero coefficients (sixteen for ZRL: fifteen here, one below), correcting the non-zero ones on the way
      for (; k <= se; ++k) {
        if (blk[k]) {
          correct(b, blk, out, k, p1);
        } else if (--r < 0) {
          break;
        }
      }
      if (k > se) {   // the run left the band
        b.st |= PR_JPEG_ST_BAD_RUN;
        return false;
      }
      if (s) {
        blk[k] = (short)val;
        out[kZigzagNatural[k]] = (short)val;
      }
      ++k;
    }
  }
  if (eobrun > 0) {
    for (; k <= se; ++k)
      if (blk[k]) correct(b, blk, out, k, p1);
    --eobrun;
  }
  return true;
}

__device__ __forceinline__ void fetch_block(const short* src, Block16* regs) {
  const Block16* s16 = (const Block16*)__builtin_assume_aligned(src, 16);
#pragma unroll
  for (int i = 0; i < 8; ++i) regs[i] = s16[i];
}

__device__ __forceinline__ void keep_block(const Block16* regs, short* blk) {
  short natural[64];
  __builtin_memcpy(natural, regs, 128);
#pragma unroll
  for (int k = 0; k < 64; ++k) blk[k] = natural[kZz[k]];
}

__global__ void __launch_bounds__(kScanThreads) jpeg_scans_entropy_kernel(ScanParams q) {
  __shared__ unsigned slices[kScanThreads * kSliceDwords];
  const JpegParams& p = q.p;
  const pr_jpeg_args& a = p.a;
  const int t = (int)blockIdx.x * p.lanes + (int)threadIdx.x;
  if ((int)threadIdx.x >= p.lanes || t >= a.n_segments) return;
  const pr_jpeg_segment sg = a.segments[t];
  if ((unsigned)sg.frame >= (unsigned)a.F) return;               // belongs to no frame of this call
  const pr_jpeg_frame& fr = a.frames[sg.frame];
  if (!frame_ok(fr, a)) return;                                   // the colour kernel reports it
  // a bad record is reported at level 0 whatever level it claims: its lane runs at no level
  const int si = q.seg_scan[t];
  if ((unsigned)si >= (unsigned)q.n_scans) {
    if (q.level == 0) atomicOr(a.status + sg.frame, (int)PR_JPEG_ST_REFUSED);
    return;
  }
  const pr_jpeg_scan sc = q.scans[si];
  const Geometry g = geometry(fr);
  const bool own = sc.ncomp == 1 && fr.ncomp == 3;   // one component of three: the blocks of its own size, one a MCU
  bool good = sc.frame == sg.frame && scan_ok(sc, fr, q);
  int across = g.mx, total = g.mx * g.my;
  if (good && own) {
    const int dw = sc.comp[0] == 0 ? fr.width : (fr.width + fr.hs - 1) / fr.hs;
    const int dh = sc.comp[0] == 0 ? fr.height : (fr.height + fr.vs - 1) / fr.vs;
    across = (dw + 7) / 8;
    total = across * ((dh + 7) / 8);
  }
  good = good && sg.begin >= 0 && sg.end <= a.data_bytes && sg.begin <= sg.end && sg.first_mcu >= 0 && sg.first_mcu < total;
  if (!good) {
    if (q.level == 0) atomicOr(a.status + sg.frame, (int)PR_JPEG_ST_REFUSED);
    return;
  }
  if (sc.level != q.level) return;
  const int n_mcus = sc.restart_interval > 0 ? min(sc.restart_interval, total - sg.first_mcu) : total - sg.first_mcu;
  const pr_jpeg_huff& tabs = a.huff[sc.huff_set];
  const int ncomp = sc.ncomp, fhs = fr.hs, fvs = fr.vs, ss = sc.ss, se = sc.se, al = sc.al;   // locals: no reload in the loop
  const int mode = ss == 0 ? (se == 63 ? 0 : (sc.ah == 0 ? 1 : 2)) : (sc.ah == 0 ? 3 : 4);
  const pr_jpeg_hufftab* dct[3];
  const pr_jpeg_hufftab* act[3];
  int comp[3];
  for (int i = 0; i < 3; ++i) {
    dct[i] = &tabs.tab[sc.dc_sel[i]];
    act[i] = &tabs.tab[2 + sc.ac_sel[i]];
    comp[i] = i < ncomp ? sc.comp[i] : 0;
  }
  short* coef = p.coef + (long)sg.frame * p.cs;
  short* blk = (short*)(slices + (int)threadIdx.x * kSliceDwords);
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
  int eobrun = 0;
  int mxi = sg.first_mcu % across, myi = sg.first_mcu / across;   // below total = across * rows
  Block16 ahead[8];
  if (mode == 4) fetch_block(coef + g.off[comp[0]] + ((long)myi * g.bw[comp[0]] + mxi) * 64, ahead);
  bool alive = true;
  for (int m = 0; m < n_mcus && alive; ++m) {
    for (int i = 0; i < ncomp && alive; ++i) {
      const int c = comp[i];
      const int hc = (c == 0 && !own) ? fhs : 1, vc = (c == 0 && !own) ? fvs : 1;
      for (int k = 0; k < hc * vc && alive; ++k) {
        // bx < g.bw[c] and by < g.bh[c]: mxi < across <= g.mx and myi < rows <= g.my, the scan's own grid inside the padded one
        const int bx = mxi * hc + (k % hc), by = myi * vc + (k / hc);
        short* out = coef + g.off[c] + ((long)by * g.bw[c] + bx) * 64;
        if (mode == 0) {
          alive = sequential_block(b, *dct[i], *act[i], pred[i], out);
        } else if (mode == 1) {
          alive = dc_first_block(b, *dct[i], al, pred[i], out);
        } else if (mode == 2) {
          // block-aligned, so coefficient 0 is the low half of an aligned dword; the bit was left 0 by the scans before
          if (get_bits(b, 1)) atomicOr((int*)out, 1 << al);
        } else if (mode == 3) {
          alive = ac_first_block(b, *act[i], ss, se, al, n_mcus - m, eobrun, out);
        } else {
          keep_block(ahead, blk);
          if (m + 1 < n_mcus) {   // one block a MCU here: the next block of the scan, in flight while this one is decoded
            const int nx = mxi + 1 == across ? 0 : mxi + 1, ny = mxi + 1 == across ? myi + 1 : myi;
            fetch_block(coef + g.off[c] + ((long)ny * g.bw[c] + nx) * 64, ahead);
          }
          alive = ac_refine_block(b, *act[i], ss, se, al, n_mcus - m, eobrun, blk, out);
        }
      }
    }
    if (++mxi == across) {
      mxi = 0;
      ++myi;
    }
  }
  if (b.st) atomicOr(a.status + sg.frame, b.st);
}

// The one clear in front of the scans: the coefficients (16 bytes a lane) and the status words.
constexpr int kClearThreads = 256;
struct ClearParams {
  Block16* coef;
  long n16;
  int* status;
  int F;
};
__global__ void __launch_bounds__(kClearThreads) jpeg_scans_clear_kernel(ClearParams c) {
  const long i = (long)blockIdx.x * kClearThreads + (long)threadIdx.x;
  if (i < c.n16) c.coef[i] = Block16{{0u, 0u, 0u, 0u}};
  if (i < c.F) c.status[i] = 0;
}

}  // namespace
}  // namespace pr

extern "C" size_t pr_jpeg_scans_workspace_bytes(int F, int H, int W) { return pr_jpeg_workspace_bytes(F, H, W); }

extern "C" int pr_jpeg_decode_scans(const pr_jpeg_scans_args* args, void* workspace, size_t workspace_bytes, void* stream) {
  using namespace pr;
  PR_REQUIRE(args, "pr_jpeg_decode_scans: null argument struct");
  const pr_jpeg_args* a = &args->base;
  PR_REQUIRE(a->F >= 0, "pr_jpeg_decode_scans: F = %d", a->F);
  if (a->F == 0) return PR_OK;
  PR_REQUIRE(a->F <= 65535, "pr_jpeg_decode_scans: F = %d frames in one call (at most 65535)", a->F);
  PR_REQUIRE(a->H >= 16 && a->W >= 16 && a->H <= 4096 && a->W <= 4096, "pr_jpeg_decode_scans: H x W = %d x %d outside 16..4096",
             a->H, a->W);
  PR_REQUIRE(a->frames, "pr_jpeg_decode_scans: null frames");
  PR_REQUIRE(a->out, "pr_jpeg_decode_scans: null out");
  PR_REQUIRE(a->status, "pr_jpeg_decode_scans: null status");
  PR_REQUIRE(a->n_segments >= 0 && a->n_huff >= 0 && a->data_bytes >= 0 && args->n_scans >= 0,
             "pr_jpeg_decode_scans: negative count (n_segments %d, n_huff %d, n_scans %d, data_bytes %lld)", a->n_segments,
             a->n_huff, args->n_scans, (long long)a->data_bytes);
  PR_REQUIRE(args->n_levels >= 0 && args->n_levels <= PR_JPEG_MAX_LEVELS, "pr_jpeg_decode_scans: n_levels = %d outside 0..%d",
             args->n_levels, PR_JPEG_MAX_LEVELS);
  PR_REQUIRE(a->n_segments == 0 || (a->segments && a->data && a->huff && a->n_huff > 0 && a->data_bytes > 0),
             "pr_jpeg_decode_scans: %d segments need data, segments and huff (null pointer, n_huff = %d or data_bytes = %lld)",
             a->n_segments, a->n_huff, (long long)a->data_bytes);
  PR_REQUIRE(a->n_segments == 0 || (args->scans && args->segment_scan && args->n_scans > 0 && args->n_levels > 0),
             "pr_jpeg_decode_scans: %d segments need scans, segment_scan and at least one level (null pointer, n_scans = %d or "
             "n_levels = %d)", a->n_segments, args->n_scans, args->n_levels);
  PR_REQUIRE(workspace, "pr_jpeg_decode_scans: null workspace");
  PR_REQUIRE(((uintptr_t)workspace & 15) == 0, "pr_jpeg_decode_scans: workspace is not 16-byte aligned");
  const size_t need = pr_jpeg_scans_workspace_bytes(a->F, a->H, a->W);
  PR_REQUIRE(workspace_bytes >= need, "pr_jpeg_decode_scans: workspace of %zu bytes, %zu needed for %d frames of %d x %d",
             workspace_bytes, need, a->F, a->H, a->W);
  const long quads = ceil_div((long)a->F * a->H * a->W, 4l);
  PR_REQUIRE(quads <= (1l << 38), "pr_jpeg_decode_scans: %d frames of %d x %d are too many pixels for one call", a->F, a->H, a->W);
  ScanParams q;
  q.p.a = *a;
  q.p.cs = padded_samples(a->H, a->W);
  q.p.out_aligned = ((uintptr_t)a->out & 3) == 0;
  q.p.lanes = 1;
  q.p.gate = nullptr;
  q.p.coef = (short*)workspace;
  q.p.planes = (unsigned char*)workspace + (size_t)a->F * q.p.cs * 2;
  q.scans = args->scans;
  q.seg_scan = args->segment_scan;
  q.n_scans = args->n_scans;
  q.n_levels = args->n_levels;
  hipStream_t s = (hipStream_t)stream;
  const long n16 = (long)a->F * q.p.cs / 8;   // cs is a multiple of 768 samples: whole 16-byte pieces
  const ClearParams clear{(Block16*)workspace, n16, a->status, a->F};
  hipLaunchKernelGGL(jpeg_scans_clear_kernel, dim3((unsigned)ceil_div(std::max(n16, (long)a->F), (long)kClearThreads)),
                     dim3(kClearThreads), 0, s, clear);
  PR_TRY(check_launch("jpeg_scans_clear_kernel"));
  if (a->n_segments > 0) {
    int cus = 0;
    PR_TRY(current_device_cus(&cus));
    q.p.lanes = std::min(kScanThreads, std::max(1, ceil_div(a->n_segments, cus * kScanWavesPerCu)));
    for (q.level = 0; q.level < q.n_levels; ++q.level) {   // one launch per level
      hipLaunchKernelGGL(jpeg_scans_entropy_kernel, dim3((unsigned)ceil_div(a->n_segments, q.p.lanes)), dim3(kScanThreads), 0, s, q);
      PR_TRY(check_launch("jpeg_scans_entropy_kernel"));
    }
  }
  return jpeg_launch_back_end(q.p, s);
}
