// The detector's convolution (det_conv.hip): fp32 MFMA implicit GEMM on NHWC, y = leaky(x * w + b) [+ res] or linear.
#pragma once
#include "common.h"

namespace pr {

struct DetConvProblem {
  const float* x = nullptr;     // [B,H,W,Cin], Cin % 4 == 0
  const float* w = nullptr;     // packed [cout_pad][kpad], k = (kh * ksize + kw) * Cin + ci (include/poserisk_hip.h, j8)
  const float* bias = nullptr;  // [cout_pad]
  const float* res = nullptr;   // [M,Cout] or nullptr: added AFTER the activation
  float* y = nullptr;           // [M,Cout]
  int B = 0, H = 0, W = 0, Cin = 0, Ho = 0, Wo = 0, Cout = 0, cout_pad = 0, kpad = 0, ksize = 1, stride = 1;
  int leaky = 1;                // 1: v > 0 ? v : 0.1f * v, 0: linear
  int out_bf16 = 0;             // 1: y is bf16[M,Cout], each value rounded once when stored (layer 0 of a bf16 handle); no res
  long M() const { return (long)B * Ho * Wo; }
  double flops() const { return 2.0 * (double)M() * Cout * ksize * ksize * Cin; }
};

// Asynchronous on `stream`; refuses by name what the kernel does not cover (a tensor of 2 GiB or more included).
int det_conv_launch(const DetConvProblem& p, hipStream_t stream);

// The bf16 convolution (det_conv_bf16.hip, section j8 "bf16"): bf16 operands on v_mfma_f32_32x32x16_bf16, fp32 accumulation,
// y = bf16 or fp32 of leaky(acc + b) [+ (float)res], rounded once.
struct DetConvBf16Problem {
  const void* x = nullptr;      // bf16[B,H,W,Cin], Cin % 8 == 0
  const void* w = nullptr;      // bf16[cout_pad][kpad], k = (kh * ksize + kw) * Cin + ci
  const float* bias = nullptr;  // f32[cout_pad]
  const void* res = nullptr;    // bf16[M,Cout] or nullptr: added in fp32 AFTER the activation, before the one rounding
  void* y = nullptr;            // bf16[M,Cout], or f32[M,Cout] with out_f32
  int B = 0, H = 0, W = 0, Cin = 0, Ho = 0, Wo = 0, Cout = 0, cout_pad = 0, kpad = 0, ksize = 1, stride = 1;
  int leaky = 1, out_f32 = 0;
  long M() const { return (long)B * Ho * Wo; }
  double flops() const { return 2.0 * (double)M() * Cout * ksize * ksize * Cin; }
};
int det_conv_bf16_launch(const DetConvBf16Problem& p, hipStream_t stream);

}  // namespace pr
