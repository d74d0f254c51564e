// The F(4x4,3x3) transform rows shared by the three-launch Winograd form (conv_winograd.hip) and the one-launch form of
// layer1 (conv_wino64.hip).  Device code only.
//
// Two sets of interpolation points (Cook-Toom on 0, +-a, +-b, infinity):
//   PTS 0 (conv form 4): a = 1, b = 2 -- Lavin & Gray's matrices,
//     B^T = [4 0 -5 0 1 0; 0 -4 -4 1 1 0; 0 4 -4 -1 1 0; 0 -2 -1 2 1 0; 0 2 -1 -2 1 0; 0 4 0 -5 0 1]
//   PTS 1 (conv form 5): a = 11/16, b = 3/2 -- points nearly reciprocal to each other keep every entry of B^T and A^T
//     within [1/3, 3.4] (Lavin's reach 5 and 8), which halves the fp32 error of a layer (scripts/wino_points.py: rms
//     error of one 3x3 layer against fp64, in units of the direct fp32 convolution's: 10.7 -> 5.4; F(2x2): 2.6).  All
//     constants are dyadic rationals, exact in fp32, so A^T [(G g) * (B^T d)] is the convolution exactly:
//     row(0) = [a^2 b^2, 0, -(a^2+b^2), 0, 1, 0]   row(+-a) = [0, -+a b^2, -b^2, +-a, 1, 0]
//     row(+-b) = [0, -+b a^2, -a^2, +-b, 1, 0]      row(inf) = [0, a^2 b^2, 0, -(a^2+b^2), 0, 1]
// kWa = 11/16, kWb = 3/2: host_plan.h (the weights' G matrix is built from the same constants)
#pragma once
#include "host_plan.h"

namespace pr {

constexpr float kWa2 = kWa * kWa, kWb2 = kWb * kWb, kWab2 = kWa2 * kWb2, kWs2 = kWa2 + kWb2;

template <int PTS, typename V>
__device__ __forceinline__ void bt6(V& a0, V& a1, V& a2, V& a3, V& a4, V& a5) {
  const V d0 = a0, d1 = a1, d2 = a2, d3 = a3, d4 = a4, d5 = a5;
  if constexpr (PTS == 0) {
    a0 = 4.f * d0 - 5.f * d2 + d4;
    a1 = (d3 + d4) - 4.f * (d1 + d2);
    a2 = 4.f * (d1 - d2) + (d4 - d3);
    a3 = 2.f * (d3 - d1) + (d4 - d2);
    a4 = 2.f * (d1 - d3) + (d4 - d2);
    a5 = 4.f * d1 - 5.f * d3 + d5;
  } else {
    const V ea = d4 - kWb2 * d2, oa = kWa * (d3 - kWb2 * d1);   // even / odd parts of the rows of +-a
    const V eb = d4 - kWa2 * d2, ob = kWb * (d3 - kWa2 * d1);   // ... of +-b
    a0 = (kWab2 * d0 - kWs2 * d2) + d4;
    a1 = ea + oa;
    a2 = ea - oa;
    a3 = eb + ob;
    a4 = eb - ob;
    a5 = (kWab2 * d1 - kWs2 * d3) + d5;
  }
}

//   A^T = [1 1 1 1 1 0; 0 a -a b -b 0; 0 a^2 a^2 b^2 b^2 0; 0 a^3 -a^3 b^3 -b^3 1]    (PTS 0: a = 1, b = 2)
template <int PTS, typename V>
__device__ __forceinline__ void at6(const V m0, const V m1, const V m2, const V m3, const V m4, const V m5, V& o0, V& o1, V& o2, V& o3) {
  const V s12 = m1 + m2, d12 = m1 - m2, s34 = m3 + m4, d34 = m3 - m4;
  o0 = (m0 + s12) + s34;
  if constexpr (PTS == 0) {
    o1 = d12 + 2.f * d34;
    o2 = s12 + 4.f * s34;
    o3 = (d12 + 8.f * d34) + m5;
  } else {
    o1 = kWa * d12 + kWb * d34;
    o2 = kWa2 * s12 + kWb2 * s34;
    o3 = ((kWa2 * kWa) * d12 + (kWb2 * kWb) * d34) + m5;
  }
}

// Column i of A^T (what plane row i adds to the four output rows): at6 one plane row at a time.
template <int PTS>
__host__ __device__ constexpr float at6_coef(int r, int i) {
  const float a = PTS == 0 ? 1.f : kWa, b = PTS == 0 ? 2.f : kWb;
  if (i == 0) return r == 0 ? 1.f : 0.f;
  if (i == 5) return r == 3 ? 1.f : 0.f;
  const float p = i == 1 ? a : i == 2 ? -a : i == 3 ? b : -b;
  return r == 0 ? 1.f : r == 1 ? p : r == 2 ? p * p : p * p * p;
}

}  // namespace pr
