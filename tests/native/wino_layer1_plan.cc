// CPU-only: which plan entries of the fp32 handle take the one-launch F(4x4,3x3) kernel of layer1 (ConvSpec::u1) and what
// they report as executed multiply-adds, for the environment the caller sets (tests/test_wino_layer1_plan.py).
//
//   wino_layer1_plan <blob.f32> <conv_form>
//
// prints one line per plan entry of stage 0 with a 3x3 kernel:  "<layer> <routed 0|1> <N3> <mfma_macs_per_frame>"
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

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  std::vector<float> blob(hmr_weight_floats());
  FILE* f = fopen(argv[1], "rb");
  if (!f || fread(blob.data(), 4, blob.size(), f) != blob.size()) return 2;
  fclose(f);
  HmrPlan plan;
  HostSink sink;
  hmr_plan_configure(&plan, 0, atoi(argv[2]), 64);
  if (hmr_plan_build(&plan, blob.data(), blob.size(), sink) != PR_OK) return 1;
  for (const ConvSpec& c : plan.convs)
    if (c.stage == 0 && c.k == 3) printf("%d %d %d %.0f\n", c.layer, c.u1 ? 1 : 0, c.N3, c.mfma_macs_per_frame(kConvBK));
  int launches = 0, wino = 0;
  hmr_plan_counts(plan, 64, 64, 1, false, &launches, &wino);
  printf("counts %d %d\n", launches, wino);
  return 0;
}
