// Device-free half of the person detector (include/poserisk_hip.h, section j8): the YOLOv3 topology table, the packed-weight
// layout, BatchNorm folding and the activation-buffer plan.  No HIP header: tests/test_detector_native.py builds det_host.cc
// with g++ under sanitizers, as tests/test_host_plan_native.py builds host_plan.cc.
#pragma once
#include <vector>

#include "host_common.h"

namespace pr {

constexpr int kDetLayers = PR_DET_NUM_LAYERS;
constexpr int kDetCoutTile = 64;   // a packed layer's rows are padded to the kernel's channel tile
constexpr int kDetKTile = 32;      // ... and its k axis to the kernel's LDS stage (det_conv.hip)
constexpr int kDetHeadChannels = 255;

// The first n layers of the table, packed offsets included (n in 1..107)
void det_topology(int n_layers, std::vector<pr_det_layer>* out);

// Which activation buffer each layer's output lives in.  A shortcut is computed by the epilogue of the convolution in front of
// it, so that convolution's own output exists only when the walk stops there (pr_det_network_until); a route of one source and
// a yolo layer are views of their source.  Buffers are reused once the last reader of their tensor has run.
struct DetPlan {
  std::vector<pr_det_layer> layers;
  std::vector<int> slot;                   // per layer: the buffer of its output (a view's is its source's)
  std::vector<size_t> slot_floats;         // per buffer: floats of one frame of the largest tensor it holds
  std::vector<int> gh, gw;                 // per layer: its output's grid
  std::vector<int> elem_bytes;             // per layer: bytes of one element of its output (4; bf16: 2, the head tensors 4)
  std::vector<size_t> slot_frame_bytes;    // per buffer: bytes of one frame of the largest tensor it holds
};
// precision 0: fp32 throughout; 1: the bf16 contract of section j8 (the same liveness walk with an element size per tensor)
int det_plan(int S_h, int S_w, DetPlan* plan, int precision = 0);

// bf16 pack (section j8, "bf16"): where each layer's bias begins in pr_det_fold_pack_bf16's blob, in BYTES (-1: no convolution)
void det_pack_offsets_bf16(int n_layers, std::vector<int64_t>* out);
// fp32 -> bf16 bits, round to nearest even on the integer; NaN stays NaN (quiet), past the largest bf16 becomes infinity
inline uint16_t bf16_rne(float v) {
  uint32_t u;
  memcpy(&u, &v, 4);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x0040u);
  u += 0x7fffu + ((u >> 16) & 1u);
  return (uint16_t)(u >> 16);
}

}  // namespace pr
