// CPU-only: what every launch of the encoder plan looks like at a given batch size -- which kernel family carries it and
// which branch of that family's launch geometry the size selects.  The kernel is hmr_route's answer (host_plan.h), the one
// the forward executes; the geometry is the launchers' own rules (hmr_split_batch, conv_tail_split, conv_regw_geometry,
// conv_panel_nsplit, the tile table), applied to the real plan (tests/test_launch_geometry.py).
//
//   launch_geometry <blob.f32> <precision 0|1> <conv_form> <max_batch> <streams> <concurrency> <B first> <B last>
//
// prints, per batch size,  "B <B> | split <serial|concurrent> <sub-batches> <equal|unequal>"  and then one line per plan entry
// and distinct sub-batch size b:  "B <B> | <layer family> | <geometry class>".  A geometry class names branches, not
// numbers: two batch sizes with the same class run the same code paths of that layer's launch.
//
//   tile kernel (conv_dma.hip, 64x64):  tiles = ceil(M / 64) (Cout / 64) groups against conv_tail_split:
//       quarters               at most 64 tiles, every one as four quarter blocks
//       whole:one-round        fewer than two whole rounds of 256 (more than 64 tiles): no quarter blocks
//       whole:exact            whole rounds, nothing remains
//       whole:big-rem          two rounds or more, more than 128 tiles remain: they run as whole tiles
//       whole+tail             two rounds or more, 1 .. 128 tiles remain: they run as quarter blocks
//     pad      the quarter blocks are padded to a multiple of 8 workgroups (the padding returns at once)
//     ragged   where the tiles of a GEMM's last, partly filled 64-row block run: none | whole | quarter | both
//   register-resident weights (conv_regw_f32.hip):  units against the persistent grid (one-unit-each | runs), whether a run
//     crosses a channel block (reloads its weights) or a group (the next GEMM of a Winograd layer), whether the last unit of a
//     GEMM is partly filled
//   Winograd layers: the transform passes' last 256-thread block partly filled or not, P % 64, then the grouped GEMM's class
//   bf16: the tile index and its ragged last block; whether layer3's plain blocks take the frame-per-workgroup kernel; balanced
//     (conv_bal_bf16.hip): channel blocks of 256 or 128, pixel runs capped by the CUs or by the pixel tiles, last 32-row tile
//     ragged or not.  The whole-Bottleneck and expansion kernels size their grids in their own launchers: not modelled
#include <set>
#include <string>

#include "native_common.h"
#include "host_plan.h"

using namespace pr;

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

static std::string fmt(const char* f, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, f);
  vsnprintf(buf, sizeof buf, f, ap);
  va_end(ap);
  return buf;
}

// conv_dma_launch on the 64x64 / 4-wave tile: `groups` GEMMs of M rows and Cout columns
static std::string dma_class(int M, int Cout, int groups, const ConvTuning& t) {
  const int tiles_n = Cout / 64, tiles_m = ceil_div(M, 64), per_group = tiles_m * tiles_n, tiles = per_group * groups;
  const ConvTailSplit s = conv_tail_split(tiles, t.tail != 0, t.tail_min_rounds, t.tail_max_rem);
  const int rounds = tiles / 256, rem = tiles % 256;
  const char* path = s.n_tail && !s.n_full ? "quarters" : s.n_tail ? "whole+tail" : rounds < t.tail_min_rounds ? "whole:one-round"
                     : rem == 0 ? "whole:exact" : "whole:big-rem";
  bool in_whole = false, in_quarter = false;
  if (M % 64)
    for (int g = 0; g < groups; ++g)
      for (int tn = 0; tn < tiles_n; ++tn) {
        const int idx = g * per_group + (tiles_m - 1) * tiles_n + tn;      // tile_ref: tile_m major inside a group
        (idx < s.n_full ? in_whole : in_quarter) = true;
      }
  const char* ragged = in_whole && in_quarter ? "both" : in_whole ? "whole" : in_quarter ? "quarter" : "none";
  return fmt("%s%s ragged=%s", path, s.n_tail && s.grid != s.n_full + s.n_tail ? " pad" : "", ragged);
}

static std::string regw_class(int M, int Cin, int Cout, int groups, const ConvTuning& t, int cus) {
  const bool grouped = groups > 1;
  const RegwGeometry g = conv_regw_geometry(M, Cin, Cout, groups, grouped ? t.regw_wt : t.regw_t, grouped ? t.regw_wnb : t.regw_nb,
                                            t.regw_per_cu, cus);
  bool xgroup = false;
  for (int wg = 0; wg < g.grid; ++wg) {
    const int u0 = conv_regw_run_begin(wg, g.units, g.grid), u1 = conv_regw_run_begin(wg + 1, g.units, g.grid);
    if (u1 > u0 && (u1 - 1) / (g.pp * g.nblk) != u0 / (g.pp * g.nblk)) xgroup = true;
  }
  return fmt("T%d NB%d %s%s%s ragged=%d", g.T, g.NB, g.units <= g.grid ? "one-unit-each" : "runs",
             conv_regw_run_crosses(g) ? " crosses-block" : "", xgroup ? " crosses-group" : "", M % (16 * g.T) != 0);
}

int main(int argc, char** argv) {
  if (argc < 9) return 2;
  const int precision = atoi(argv[2]), form = atoi(argv[3]), max_batch = atoi(argv[4]), streams = atoi(argv[5]),
            concurrency = atoi(argv[6]), b_first = atoi(argv[7]), b_last = atoi(argv[8]);
  std::vector<float> blob(hmr_weight_floats());
  FILE* f = fopen(argv[1], "rb");
  if (!f || fread(blob.data(), 4, blob.size(), f) != blob.size()) return 2;
  fclose(f);
  HmrPlan plan;
  HostSink sink;
  hmr_plan_configure(&plan, precision, form, max_batch);
  if (hmr_plan_build(&plan, blob.data(), blob.size(), sink) != PR_OK) return 1;
  ConvTuning tune;                                          // the defaults, as conv_tuning_from_env leaves them in a clean environment
  if (concurrency >= 2) tune.regw_per_cu = 1;               // pr_hmr_set_concurrency
  const int n_chunks = std::max(1, std::min(std::min(streams, kHmrMaxChunks), max_batch));      // pr_hmr_set_streams
  const int chunk_cap = hmr_chunk_cap(max_batch, n_chunks);
  const bool bf = precision == 1;
  for (int B = b_first; B <= b_last; ++B) {
    std::vector<int> sizes((size_t)std::max(n_chunks, ceil_div(B, chunk_cap)) + 1);
    bool concurrent = false;
    const int n = hmr_split_batch(B, chunk_cap, n_chunks, false, sizes.data(), (int)sizes.size(), &concurrent);
    const std::set<int> distinct(sizes.begin(), sizes.begin() + n);
    printf("B %d | split %s %d %s\n", B, concurrent ? "concurrent" : "serial", n, distinct.size() == 1 ? "equal" : "unequal");
    for (int b : distinct)
      for (size_t ci = 0; ci < plan.convs.size();) {
        const HmrRoute rt = hmr_route(plan, tune, ci, b);
        const ConvSpec& c = *rt.spec;
        ci += rt.span;
        if (rt.span == 3) {                 // a block the frame-per-workgroup kernel has taken
          printf("B %d | block %d @%d | bottleneck256 frame-per-workgroup %s\n", B, c.Cin, c.H, b <= plan.cus ? "one-round" : "rounds");
          continue;
        }
        const int M = b * c.Ho() * c.Wo();
        const std::string fam = fmt("k%d s%d %d%s->%d @%d%s%s", c.k, c.stride, c.Cin, c.in2_buf >= 0 ? fmt("+%d", c.Cin2).c_str() : "",
                                    c.N3 ? c.N3 : c.Cout, c.H, c.res_buf >= 0 || c.res3_buf >= 0 ? " +res" : "", c.N3 ? " +conv3" : "");
        std::string cls;
        switch (rt.kernel) {
          case HmrKernel::StemPool: cls = "stem_pool"; break;
          case HmrKernel::Bottleneck: cls = fmt("bottleneck%d%s", c.bneck_planes, c.bneck_first ? " first" : ""); break;
          case HmrKernel::Wino64: cls = "wino64"; break;
          case HmrKernel::Winograd: {
            const int m = c.wino_m, P = b * ((c.H + m - 1) / m) * ((c.W + m - 1) / m), per = m == 4 ? tune.wino_vec : 4;
            ConvShape g;                    // the grouped GEMM, as conv_winograd_launch hands it on
            g.groups = (m + 2) * (m + 2); g.M = P; g.Cin = c.Cin; g.Cout = c.Cout;
            cls = fmt("winograd%d xform-ragged=%d,%d P%%64=%d | ", c.wino_form, (long)P * (c.Cin / per) % 256 != 0,
                      (long)P * (c.Cout / per) % 256 != 0, P % 64 != 0) +
                  (tune.wino_regw && conv_regw_f32_fits(g) ? "regw " + regw_class(P, c.Cin, c.Cout, g.groups, tune, plan.cus)
                                                           : "tile " + dma_class(P, c.Cout, g.groups, tune));
            break;
          }
          case HmrKernel::Fused3: cls = fmt("fused3 ragged=%d", M % 64 != 0); break;
          case HmrKernel::RegW: cls = "regw " + regw_class(M, c.Cin, c.Cout, 1, tune, plan.cus); break;
          case HmrKernel::Panel: cls = fmt("panel nsplit=%d ragged=%d", conv_panel_nsplit(ceil_div(M, 64), c.Cout / 64), M % 64 != 0); break;
          case HmrKernel::Expand: cls = "expand"; break;
          case HmrKernel::Balanced: {
            const int wide = c.Cout % 256 == 0 ? 256 : 128, by_cus = std::max(plan.cus / (8 * (c.Cout / wide)), 1);
            cls = fmt("balanced nb%d runs=%s ragged=%d", wide, std::max(ceil_div(M, 32) / 8, 1) < by_cus ? "tiles" : "cus", M % 32 != 0);
            break;
          }
          case HmrKernel::Tile:
            cls = bf ? fmt("tile cfg%d ragged=%d", rt.cfg, M % conv_tile_cfg(rt.cfg)->BM != 0) : c.splitk > 1 ? "tile split-k" : "tile " + dma_class(M, c.Cout, 1, tune);
            break;
        }
        printf("B %d | %s | %s\n", B, fam.c_str(), cls.c_str());
      }
  }
  return 0;
}
