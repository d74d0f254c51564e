// jpeg_host_shim.h for csrc/jpeg_scans.hip: that file's refinement procedure keeps a per-lane copy of the block in LDS.  On the
// host a workgroup's threads run one after the other and a lane only ever touches its own slice, so the LDS array is a static
// array.  tests/test_jpeg_scans_native.py copies this file as common.h beside jpeg_host_shim.h.
#pragma once
#include "jpeg_host_shim.h"

#define __shared__ static
