// The library's one device allocator, and the internal fence behind POSERISK_FENCE (DESIGN.md "The internal fence").
//
// The guard-band tests (tests/guard_band.py) fence the tensors a caller hands in; the workspaces the handles and the
// stand-alone entries allocate themselves -- activations, Winograd V / M, split-K slab, packed weights, regressor and SMPL
// workspaces -- are out of their reach.  Every one of those allocations goes through device_alloc below.
//
//   mode 0 (switch unset or 0)  device_alloc is the hipMalloc it replaces and device_free the hipFree: nothing recorded.
//   mode 1 (head) / 2 (tail)    guard | payload | guard, all 0xFF before use, recorded under a name; pr_fence_check reads
//                               the guards back.  The two modes allocate alike; where a tensor is placed inside a buffer
//                               that is sized as a maximum (first byte on the payload's first: head; last byte on the
//                               payload's last: tail) is the owner's business (hmr.hip: `placed`).
#pragma once
#include "common.h"

namespace pr {

// POSERISK_FENCE as a handle reads it at create (a stand-alone entry: per call): 0, 1 or 2
int fence_mode_from_env();

// `bytes` of device memory.  mode != 0: between guards of fence_guard_bytes(frame_bytes) (frame_bytes = one frame of the
// largest tensor the buffer holds; 0 = no frame axis), recorded under the printf-style name.
int device_alloc(void** out, size_t bytes, int mode, size_t frame_bytes, const char* name_fmt, ...)
    __attribute__((format(printf, 5, 6)));
// Frees what device_alloc returned.  A fenced allocation's guards are read once more first: what they show is kept until
// the next pr_fence_check reports it.
void device_free(void* p);
// Renames a fenced allocation (the plan's constants get their names once the plan knows whose they are); no-op otherwise
void fence_rename(const void* p, const char* name_fmt, ...) __attribute__((format(printf, 2, 3)));

}  // namespace pr
