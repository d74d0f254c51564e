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
};
int det_plan(int S_h, int S_w, DetPlan* plan);

}  // namespace pr
