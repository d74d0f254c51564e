// The bf16 fold + pack of the person detector (csrc/det_host.cc, pr_det_fold_pack_bf16) as a stand-alone program, for a build
// under ASan + UBSan (tests/test_detector_bf16_native.py): the fold of a (truncated) table into an exact-size
// heap block that is NOT aligned beyond a byte, the refusals by name, the rounding rule on its edge cases, and the bf16 plan's
// buffers checked against every tensor's size in bytes.
//   det_pack_bf16_check <n_layers> <weights.f32> <bn_eps> <packed_out.bin>
#include <cmath>
#include <limits>
#include <string>

#define NATIVE_QUIET_ERRORS    // the refusals are provoked on purpose and their messages read
#include "native_common.h"
#include "det_host.h"

static float from_bits(uint32_t u) {
  float f;
  memcpy(&f, &u, 4);
  return f;
}
static bool refused(int status, const char* name) { return status == PR_ERR_INVALID && strstr(pr::g_error, name) != nullptr; }

int main(int argc, char** argv) {
  if (argc != 5) return 2;
  const int n_layers = atoi(argv[1]);
  const double eps = atof(argv[3]);

  // the rounding rule: ties to even in both directions, NaN stays NaN, past the largest bf16 becomes infinity
  CHECK(pr::bf16_rne(from_bits(0x3f808000u)) == 0x3f80, "a tie rounds down to the even neighbour");
  CHECK(pr::bf16_rne(from_bits(0x3f818000u)) == 0x3f82, "a tie rounds up to the even neighbour");
  CHECK(pr::bf16_rne(from_bits(0x3f808001u)) == 0x3f81 && pr::bf16_rne(from_bits(0x3f817fffu)) == 0x3f81, "off a tie: to nearest");
  CHECK(pr::bf16_rne(from_bits(0x7f7fffffu)) == 0x7f80 && pr::bf16_rne(from_bits(0xff7f8000u)) == 0xff80, "overflow gives infinity");
  CHECK(pr::bf16_rne(from_bits(0x7f800001u)) == 0x7fc0 && pr::bf16_rne(from_bits(0xffc12345u)) == 0xffc1, "NaN stays NaN");
  CHECK(pr::bf16_rne(from_bits(0x80000000u)) == 0x8000 && pr::bf16_rne(from_bits(0x00008000u)) == 0x0000, "zeros and a denormal tie");

  const size_t nw = pr_det_weight_floats(n_layers), nb = pr_det_packed_bytes_bf16(n_layers);
  CHECK(nb > 0 && nb % 16 == 0, "packed bytes %zu", nb);
  CHECK(pr_det_packed_bytes_bf16(0) == 0 && pr_det_packed_bytes_bf16(108) == 0, "counts outside 1..107");
  std::vector<float> w(nw);
  FILE* f = fopen(argv[2], "rb");
  if (!f || fread(w.data(), sizeof(float), nw, f) != nw) return 3;
  fclose(f);
  // exact size, one byte into a heap block: a write one byte off either end, or an aligned wide store, is the sanitizer's
  std::vector<unsigned char> block(nb + 1);
  unsigned char* packed = block.data() + 1;
  CHECK(pr_det_fold_pack_bf16(n_layers, w.data(), nw, eps, packed, nb) == PR_OK, "fold_pack_bf16: %s", pr::g_error);
  f = fopen(argv[4], "wb");
  if (!f || fwrite(packed, 1, nb, f) != nb) return 4;
  fclose(f);
  CHECK(refused(pr_det_fold_pack_bf16(0, w.data(), nw, eps, packed, nb), "n_layers = 0"), "n_layers = 0: %s", pr::g_error);
  CHECK(refused(pr_det_fold_pack_bf16(108, w.data(), nw, eps, packed, nb), "n_layers = 108"), "n_layers = 108: %s", pr::g_error);
  CHECK(refused(pr_det_fold_pack_bf16(n_layers, nullptr, nw, eps, packed, nb), "null weights_host"), "null weights: %s", pr::g_error);
  CHECK(refused(pr_det_fold_pack_bf16(n_layers, w.data(), nw, eps, nullptr, nb), "null packed_host"), "null packed: %s", pr::g_error);
  CHECK(refused(pr_det_fold_pack_bf16(n_layers, w.data(), nw - 1, eps, packed, nb), "n_floats ="), "a short body: %s", pr::g_error);
  CHECK(refused(pr_det_fold_pack_bf16(n_layers, w.data(), nw, eps, packed, nb + 2), "packed_bytes ="), "a wrong capacity: %s",
        pr::g_error);
  CHECK(refused(pr_det_fold_pack_bf16(n_layers, w.data(), nw, 0.0, packed, nb), "bn_eps = 0"), "bn_eps = 0: %s", pr::g_error);
  CHECK(refused(pr_det_fold_pack_bf16(n_layers, w.data(), nw, 1.0, packed, nb), "bn_eps = 1"), "bn_eps = 1: %s", pr::g_error);

  // byte offsets: consecutive, 16-byte aligned, ending on the blob's size
  std::vector<int64_t> off;
  pr::det_pack_offsets_bf16(PR_DET_NUM_LAYERS, &off);
  std::vector<pr_det_layer> table;
  pr::det_topology(PR_DET_NUM_LAYERS, &table);
  int64_t at = 0;
  for (int l = 0; l < PR_DET_NUM_LAYERS; ++l) {
    if (table[l].type != PR_DET_CONV) {
      CHECK(off[l] == -1, "layer %d has an offset", l);
      continue;
    }
    CHECK(off[l] == at && at % 16 == 0, "offset of layer %d: %lld for %lld", l, (long long)off[l], (long long)at);
    at += (int64_t)table[l].cout_pad * 4 + (int64_t)table[l].cout_pad * table[l].kpad * (l == 0 ? 4 : 2);
    CHECK(l == 0 || table[l].cin % 32 == 0, "layer %d: Cin %d is padded in k", l, table[l].cin);
  }
  CHECK((size_t)at == pr_det_packed_bytes_bf16(PR_DET_NUM_LAYERS), "the offsets end on the blob's size");

  // the bf16 plan: the fp32 plan's buffers with an element size per tensor; the head tensors keep 4 bytes
  const int sizes[][2] = {{32, 32}, {32, 64}, {64, 96}, {256, 416}, {416, 416}};
  for (const auto& s : sizes) {
    pr::DetPlan P32, P16;
    CHECK(pr::det_plan(s[0], s[1], &P32) == PR_OK && pr::det_plan(s[0], s[1], &P16, 1) == PR_OK, "det_plan: %s", pr::g_error);
    CHECK(P32.slot == P16.slot && P32.slot_floats == P16.slot_floats, "%dx%d: the two plans place their tensors differently", s[0], s[1]);
    for (int l = 0; l < PR_DET_NUM_LAYERS; ++l) {
      const bool head = l == 81 || l == 82 || l == 93 || l == 94 || l == 105 || l == 106;
      CHECK(P32.elem_bytes[l] == 4 && P16.elem_bytes[l] == (head ? 4 : 2), "element size of layer %d", l);
      const size_t elems = (size_t)P16.gh[l] * P16.gw[l] * table[l].cout;
      CHECK(P16.slot_frame_bytes[P16.slot[l]] >= elems * P16.elem_bytes[l] && P32.slot_frame_bytes[P32.slot[l]] >= elems * 4,
            "%dx%d: layer %d does not fit its buffer", s[0], s[1], l);
    }
    for (size_t b = 0; b < P32.slot_floats.size(); ++b)
      CHECK(P32.slot_frame_bytes[b] == 4 * P32.slot_floats[b] && P16.slot_frame_bytes[b] <= P32.slot_frame_bytes[b], "buffer %zu", b);
  }
  pr::DetPlan P;
  CHECK(refused(pr::det_plan(64, 96, &P, 2), "precision = 2"), "precision 2: %s", pr::g_error);
  printf("det_pack_bf16_check: %zu floats packed to %zu bytes, %d failures\n", nw, nb, g_fail);
  return g_fail ? 1 : 0;
}
