// CPU-only check of the internal fence's device-free part (csrc/host_common.h: fence_guard_bytes, fence_tail_offset,
// fence_scan; csrc/host_plan.h: the byte sizes hmr.hip places every tensor by), built by tests/test_internal_fence_cpu.py with
// g++ under ASan + UBSan.
//
//   fence_check <blob.f32>
//
//   * guard sizes over a range of frame sizes: a multiple of 4096 bytes, never below 64 KiB, never below the frame;
//   * tail placement: for the three configurations of tests/geometry_classes.py (fp32 default form, fp32 direct, bf16), a handle
//     of capacity 256 and B in {1, 37, 217, 256}, the plan is walked launch by launch as hmr_route (host_plan.h) routes it at that B.  Every
//     tensor a launch reads or writes: fits its buffer, has a non-negative offset that is a multiple of 256 bytes, ends on
//     the buffer's last byte; and what a consumer computes for its input is what the producer computed when it wrote that
//     buffer (the stem's input, residuals, the second source of a dual-source conv3, the whole-block alternates of layer3,
//     the average pool, the taps of pr_hmr_encode_until, V / M of the Winograd layers, the split-K slab);
//   * fence_scan on host copies of a guard with no byte, one byte, the first byte, the last byte and a run of bytes changed.
#include <string>

#include "native_common.h"
#include "host_plan.h"

using namespace pr;

static long g_checked = 0;

struct HostSink : PlanSink {
  std::vector<void*> blocks;
  int upload(const void* host, size_t bytes, float** out) override {
    (void)host;
    return zeros(bytes, out);      // the contents are test_host_plan_native's business
  }
  int zeros(size_t bytes, float** out) override {
    blocks.push_back(calloc(1, bytes ? bytes : 1));
    *out = static_cast<float*>(blocks.back());
    return PR_OK;
  }
  ~HostSink() override {
    for (void* p : blocks) free(p);
  }
};

static void check_guards() {
  const size_t frames[] = {0, 1, 4095, 4096, 4097, 65535, 65536, 65537, 100352, 802816, (size_t)112 * 112 * 64 * 2, (size_t)112 * 112 * 64 * 4,
                           (size_t)36 * 49 * 256 * 4 + 12};
  for (size_t f : frames) {
    const size_t g = fence_guard_bytes(f);
    CHECK(g % 4096 == 0 && g >= ((size_t)64 << 10) && g >= f && g < std::max<size_t>(f, (size_t)64 << 10) + 4096, "guard of a %zu-byte frame is %zu", f, g);
  }
  for (size_t f = 0; f < 200000; f += 777) CHECK(fence_guard_bytes(f) % 4096 == 0 && fence_guard_bytes(f) >= std::max<size_t>(f, 65536), "guard(%zu)", f);
}

// one tensor in a buffer of `cap` bytes, tail mode
static void check_place(const char* tag, const char* what, size_t ci, size_t cap, size_t bytes) {
  bool ok = true;
  const size_t off = fence_tail_offset(cap, bytes, &ok);
  ++g_checked;
  CHECK(bytes > 0 && bytes <= cap, "%s entry %zu %s: %zu bytes in a buffer of %zu", tag, ci, what, bytes, cap);
  CHECK(ok, "%s entry %zu %s: %zu bytes of %zu: refused (no multiple of 256, or too large)", tag, ci, what, bytes, cap);
  CHECK(off + bytes == cap && off % 256 == 0 && off <= cap, "%s entry %zu %s: offset %zu + %zu != %zu", tag, ci, what, off, bytes, cap);
}

static void walk(const HmrPlan& pl, const HmrChunkSizes& z, int B, const char* tag) {
  const int prec = pl.precision;
  size_t holds[6] = {};      // bytes of the tensor each activation buffer holds, as its producer placed it
  auto reads = [&](size_t ci, const char* what, int buf, size_t bytes) {
    check_place(tag, what, ci, hmr_act_capacity_bytes(z, buf), bytes);
    CHECK(holds[buf] == bytes, "%s entry %zu reads %s from buffer %d as %zu bytes, its producer wrote %zu", tag, ci, what, buf, bytes, holds[buf]);
  };
  auto writes = [&](size_t ci, const char* what, int buf, size_t bytes) {
    check_place(tag, what, ci, hmr_act_capacity_bytes(z, buf), bytes);
    holds[buf] = bytes;
  };
  size_t tapped[HmrPlan::kBlocks] = {};
  holds[0] = hmr_conv_tensor_bytes(pl.convs[0], prec, B).x;      // the layout change (stem_in_at)
  const size_t pooled = hmr_act_bytes(prec, B, 56, 56, 64);
  const ConvTuning tune;
  for (size_t ci = 0, span = 1; ci < pl.convs.size(); ci += span) {
    const ConvSpec& c = pl.convs[ci];
    const ConvTensorBytes t = hmr_conv_tensor_bytes(c, prec, B);
    const HmrRoute rt = hmr_route(pl, tune, ci, B);
    span = (size_t)rt.span;
    if (c.alt3 >= 0) {      // the whole-block alternate of entries ci .. ci + 2: same input, and the output the third one writes
      const ConvSpec& blk = pl.fused3[c.alt3].blk;
      const ConvTensorBytes a = hmr_conv_tensor_bytes(blk, prec, B);
      reads(ci, "block256 x", blk.in_buf, a.x);
      const ConvSpec& last = pl.convs[ci + 2];
      CHECK(blk.out_buf == last.out_buf && a.y == hmr_conv_tensor_bytes(last, prec, B).y, "%s entry %zu: block256 writes another tensor than conv3", tag, ci);
      check_place(tag, "block256 y", ci, hmr_act_capacity_bytes(z, blk.out_buf), a.y);
      if (rt.span == 3) writes(ci, "block256 y", blk.out_buf, a.y);      // at this B it is the launch that runs, entries ci .. ci + 2 do not
    }
    if (rt.span == 3) CHECK(rt.spec == &pl.fused3[c.alt3].blk, "%s entry %zu: three entries taken by another spec than their alternate", tag, ci);
    else if (rt.kernel == HmrKernel::StemPool) {      // stem + max-pool in one launch: act[0] -> act[2]
      reads(ci, "stem x", 0, t.x);
      writes(ci, "stem-pool y", 2, pooled);
    } else {
      reads(ci, "x", c.in_buf, t.x);
      if (c.res_buf >= 0) reads(ci, "res", c.res_buf, t.y);
      if (c.in2_buf >= 0) reads(ci, "x2", c.in2_buf, t.x2);
      if (c.w3 && c.out3_buf >= 0) {
        if (c.res3_buf >= 0) reads(ci, "res3", c.res3_buf, t.y3);
        writes(ci, "y3", c.out3_buf, t.y3);
      } else {
        writes(ci, "y", c.out_buf, t.y);
      }
      if (ci == 0) {      // the separate max-pool: act[1] -> act[2]
        reads(ci, "max-pool x", 1, hmr_act_bytes(prec, B, 112, 112, 64));
        writes(ci, "max-pool y", 2, pooled);
      }
    }
    if (c.u) {
      check_place(tag, "wino V|M", ci, z.wino_floats * sizeof(float), hmr_wino_work_floats(c, B) * sizeof(float));
      const size_t tiles = (size_t)B * ((c.H + c.wino_m - 1) / c.wino_m) * ((c.W + c.wino_m - 1) / c.wino_m);
      CHECK(hmr_wino_work_floats(c, B) == (size_t)(c.wino_m + 2) * (c.wino_m + 2) * tiles * (c.Cin + c.Cout), "%s entry %zu: wino work", tag, ci);
    }
    if (c.splitk > 1) {
      const size_t tiles = (size_t)ceil_div(B * c.Ho() * c.Wo(), 64) * (c.Cout / 64);
      check_place(tag, "split-K slab", ci, z.slab_floats * sizeof(float), tiles * c.splitk * 4096 * sizeof(float));
    }
    for (int k = 0; k < HmrPlan::kBlocks; ++k)
      if ((size_t)pl.block_last[k] >= ci && (size_t)pl.block_last[k] < ci + span) tapped[k] = holds[pl.block_buf[k]];
  }
  reads(pl.convs.size(), "average pool x", pl.final_buf, hmr_act_bytes(prec, B, 7, 7, 2048));
  for (int k = 0; k < HmrPlan::kBlocks; ++k)
    CHECK(tapped[k] == (size_t)B * hmr_block_frame_elems(k) * (prec == 1 ? 2 : 4), "%s: the tap of block %d copies %zu bytes, the block wrote %zu", tag, k,
          (size_t)B * hmr_block_frame_elems(k) * (prec == 1 ? 2 : 4), tapped[k]);
}

static void check_tail_offsets(const std::vector<float>& blob) {
  // fence_tail_offset itself
  bool ok = true;
  CHECK(fence_tail_offset(4096, 4096, &ok) == 0 && ok, "a full buffer sits at offset 0");
  CHECK(fence_tail_offset(4096, 256, &ok) == 3840 && ok, "256 of 4096");
  ok = true;
  (void)fence_tail_offset(4096, 100, &ok);
  CHECK(!ok, "100 bytes are no multiple of 256");
  ok = true;
  CHECK(fence_tail_offset(4096, 8192, &ok) == 0 && !ok, "a tensor larger than its buffer is refused at offset 0");
  // tests/geometry_classes.py CONFIGS: (precision, conv_form); + split-K on, which alone allocates the slab
  const struct { const char* name; int precision, form, splitk; } configs[] = {
      {"fp32_default", 0, -1, 1}, {"fp32_direct", 0, 0, 1}, {"bf16", 1, -1, 1}, {"fp32_direct_splitk", 0, 0, 3}};
  const int cap = 256, batches[] = {1, 37, 217, 256};      // 217: the last B at which layer3's plain bf16 blocks are three launches, 256: one
  for (const auto& cf : configs) {
    HmrPlan plan;
    HostSink sink;
    hmr_plan_configure(&plan, cf.precision, cf.form, cap);
    plan.splitk = cf.splitk;
    if (hmr_plan_build(&plan, blob.data(), blob.size(), sink) != PR_OK) {
      CHECK(false, "%s: the plan does not build", cf.name);
      continue;
    }
    const HmrChunkSizes z = hmr_chunk_sizes(plan, hmr_chunk_cap(cap, 1));
    bool any_wino = false, any_split = false;
    for (const ConvSpec& c : plan.convs) {
      any_wino = any_wino || c.u;
      any_split = any_split || c.splitk > 1;
    }
    CHECK(any_wino == (cf.precision == 0 && cf.form != 0) && any_split == (cf.splitk > 1), "%s: unexpected routes", cf.name);
    for (int B : batches) {
      char tag[64];
      snprintf(tag, sizeof tag, "%s B=%d", cf.name, B);
      walk(plan, z, B, tag);
    }
  }
}

static void check_scan() {
  const size_t n = 65536;
  std::vector<unsigned char> g(n, 0xFF);      // exact size: ASan sees a scan that runs past it
  FenceScan s = fence_scan(g.data(), n);
  CHECK(s.count == 0, "an untouched guard scans as touched");
  s = fence_scan(g.data(), 0);
  CHECK(s.count == 0, "an empty guard scans as touched");
  g[1234] = 0;
  s = fence_scan(g.data(), n);
  CHECK(s.count == 1 && s.first == 1234 && s.last == 1234, "one byte: %zu %zu %zu", s.count, s.first, s.last);
  g[1234] = 0xFF;
  g[0] = 0xFE;
  s = fence_scan(g.data(), n);
  CHECK(s.count == 1 && s.first == 0 && s.last == 0, "the first byte: %zu %zu %zu", s.count, s.first, s.last);
  g[0] = 0xFF;
  g[n - 1] = 0x7F;
  s = fence_scan(g.data(), n);
  CHECK(s.count == 1 && s.first == n - 1 && s.last == n - 1, "the last byte: %zu %zu %zu", s.count, s.first, s.last);
  g[n - 1] = 0xFF;
  for (size_t i = 300; i < 812; ++i) g[i] = (unsigned char)(i % 255);      // a run of 512 bytes, none of them 0xFF
  s = fence_scan(g.data(), n);
  CHECK(s.count == 512 && s.first == 300 && s.last == 811, "a run: %zu %zu %zu", s.count, s.first, s.last);
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  std::vector<float> blob(hmr_weight_floats());
  FILE* f = fopen(argv[1], "rb");
  if (!f || fread(blob.data(), 4, blob.size(), f) != blob.size()) return 2;
  fclose(f);
  check_guards();
  check_tail_offsets(blob);
  check_scan();
  printf("fence_check: %ld tensors placed, %d failures\n", g_checked, g_fail);
  return g_fail ? 1 : 0;
}
