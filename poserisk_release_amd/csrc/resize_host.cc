// Host half of the frame downscale (include/poserisk_hip.h, section j3): the per-axis tap tables of the integer bilinear
// contract.  No device call and no HIP header: tests/test_frontend_native.py builds this file with g++ under sanitizers.
#include <cmath>

#include "host_common.h"

// the position is a product and a difference rounded separately, never one fused operation
#pragma STDC FP_CONTRACT OFF

namespace pr {
namespace {

// One axis: S source samples -> d destination samples.  ofs[i] = the first tap, coef[2 i], coef[2 i + 1] = the two weights
// (of 2048).  The expressions are the contract's, written in the precision it names: the position in double, rounded to
// float once, the fraction and the weights in float.
void resize_axis(int S, int d, int32_t* ofs, int16_t* coef) {
  const double scale = 1.0 / ((double)d / S);
  for (int i = 0; i < d; ++i) {
    float f = (float)((i + 0.5) * scale - 0.5);
    int s = (int)std::floor(f);
    f -= (float)s;
    if (s < 0) s = 0, f = 0.f;
    if (s >= S - 1) s = S - 1, f = 0.f;
    ofs[i] = s;
    const float w0 = (1.f - f) * 2048.f, w1 = f * 2048.f;   // exact products: a power of two
    coef[2 * i] = (int16_t)std::nearbyint(w0);               // round to nearest even (the default rounding mode)
    coef[2 * i + 1] = (int16_t)std::nearbyint(w1);
  }
}

}  // namespace
}  // namespace pr

extern "C" int pr_resize_plan(int H, int W, int h, int w, int32_t* xofs_host, int16_t* xcoef_host, int32_t* yofs_host,
                              int16_t* ycoef_host, int32_t* mode_host) {
  using namespace pr;
  PR_REQUIRE(H >= 1 && H <= PR_RESIZE_MAX_SIDE && W >= 1 && W <= PR_RESIZE_MAX_SIDE && h >= 1 && h <= PR_RESIZE_MAX_SIDE &&
                 w >= 1 && w <= PR_RESIZE_MAX_SIDE,
             "pr_resize_plan: %d x %d -> %d x %d: every side must lie in 1..%d", W, H, w, h, PR_RESIZE_MAX_SIDE);
  PR_REQUIRE(xofs_host, "pr_resize_plan: null xofs_host");
  PR_REQUIRE(xcoef_host, "pr_resize_plan: null xcoef_host");
  PR_REQUIRE(yofs_host, "pr_resize_plan: null yofs_host");
  PR_REQUIRE(ycoef_host, "pr_resize_plan: null ycoef_host");
  PR_REQUIRE(mode_host, "pr_resize_plan: null mode_host");
  resize_axis(W, w, xofs_host, xcoef_host);
  resize_axis(H, h, yofs_host, ycoef_host);
  *mode_host = (H == h && W == w) ? PR_RESIZE_COPY : (W == 2 * w && H == 2 * h) ? PR_RESIZE_HALF : PR_RESIZE_LINEAR;
  return PR_OK;
}
