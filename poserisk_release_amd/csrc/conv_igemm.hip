// Host side of the convolution launches: the A/B switches' environment and the dispatch to the LDS-DMA kernels (conv_dma.hip,
// conv_dma_bf16.hip), the fused kernels (conv_fused.hip), the row-panel form and the persistent kernels.  The tile table and
// the choice of a tile (conv_pick_tile_cfg) are device-free code: host_plan.cc.
#include "conv_igemm.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

namespace pr {

ConvTuning conv_tuning_from_env() {
  ConvTuning t;
  if (const char* e = getenv("POSERISK_CONV_CFG")) t.force_cfg = atoi(e);
  if (const char* e = getenv("POSERISK_CONV_TAIL")) t.tail = atoi(e);
  if (const char* e = getenv("POSERISK_TAIL_MIN_ROUNDS")) t.tail_min_rounds = atoi(e);
  if (const char* e = getenv("POSERISK_TAIL_MAX_REM")) t.tail_max_rem = atoi(e);
  if (const char* e = getenv("POSERISK_WINO_VEC")) t.wino_vec = atoi(e) == 4 ? 4 : 2;
  if (const char* e = getenv("POSERISK_WINO_REGW")) t.wino_regw = atoi(e) != 0;
  if (const char* e = getenv("POSERISK_REGW_PER_CU")) { const int v = atoi(e); if (v >= 1 && v <= 4) t.regw_per_cu = v; }
  if (const char* e = getenv("POSERISK_REGW_T")) t.regw_t = atoi(e);
  if (const char* e = getenv("POSERISK_REGW_NB")) t.regw_nb = atoi(e);
  if (const char* e = getenv("POSERISK_REGW_WT")) t.regw_wt = atoi(e);
  if (const char* e = getenv("POSERISK_REGW_WNB")) t.regw_wnb = atoi(e);
  if (const char* e = getenv("POSERISK_WINO_TILE")) {
    int bm = 0, bn = 0;
    if (sscanf(e, "%dx%d", &bm, &bn) == 2 && (bm == 64 || bm == 128) && (bn == 64 || bn == 128)) { t.wino_bm = bm; t.wino_bn = bn; }
  }
  if (const char* e = getenv("POSERISK_BAL_STAGES")) t.bal_stages = atoi(e);   // 4, 5, or 6 = ring of five with paired stages
  return t;
}

int conv_launch(const ConvProblem& p, int cfg, hipStream_t stream) {
  if (cfg == kConvCfgPanel) return conv_panel_launch(p, stream);
  if (cfg == kConvCfgRegW) return conv_regw_f32_launch(p, stream);
  if (cfg == kConvCfgBalanced || cfg == kConvCfgBalanced + 1) return conv_bal_bf16_launch(p, stream, cfg - kConvCfgBalanced);
  if (cfg == kConvCfgExpand) {
    PR_REQUIRE(p.precision == 1 && p.KH == 1 && p.KW == 1 && p.stride == 1 && p.pad == 0 && p.bias && !p.w3 && p.groups == 1 &&
                   (p.x2 != nullptr) != (p.res != nullptr),
               "conv: tile cfg %d is the bf16 1x1 expansion with register-resident weights: + bias + residual, or + a second "
               "source without residual", cfg);
    if (p.x2)
      return expand_dual_bf16_launch(p.x, p.x2, p.w, p.bias, p.y, p.B, p.Ho, p.Wo, p.H2, p.W2, p.stride2, p.Cin, p.Cin2, p.Cout,
                                     p.relu, stream);
    return expand_res_bf16_launch(p.x, p.w, p.bias, p.res, p.y, (long)p.M(), p.Cin, p.Cout, p.relu, stream);
  }
  PR_REQUIRE(conv_tile_cfg(cfg), "conv: bad tile cfg %d", cfg);
  const ConvTileCfg& t = *conv_tile_cfg(cfg);
  if (p.w3) return conv_fused3_launch(p, stream);
  // a tile that does not fit the layer is refused as such, retired or not; a retired one that fits is refused by name
  PR_REQUIRE(p.Cout % t.BN == 0, "conv: Cout %d not a multiple of tile N %d", p.Cout, t.BN);
  PR_REQUIRE(t.live, "conv: tile cfg %d (%s) is retired", cfg, t.name);
  if (p.precision == 1) return conv_dma_bf16_launch(p, t.BM, t.BN, stream, t.threads);
  PR_REQUIRE(p.KH == p.KW, "conv: square kernels only (got %dx%d)", p.KH, p.KW);
  PR_REQUIRE(p.Cin % 4 == 0, "conv: Cin %% 4 != 0 (%d)", p.Cin);
  PR_REQUIRE(p.x && p.w && p.y, "conv: null tensor");
  return conv_dma_launch(p, t.BM, t.BN, stream, t.threads);
}

}  // namespace pr
