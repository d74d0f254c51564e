"""The internal fence's device-free part under ASan + UBSan, on the CPU.

POSERISK_FENCE (DESIGN.md "The internal fence") puts every device allocation of the library's own between guards and, in tail
mode, ends every tensor of the encoder's workspaces on its buffer's last byte.  What decides that without a device -- the
guard size, the tail offset, the scan of a guard's host copy (csrc/host_common.h) and the byte sizes hmr.hip places each
tensor by (csrc/host_plan.h) -- is held here by a stand-alone program, tests/native/fence_check.cc (its header lists the
checks): guard sizes, the tail placement of every tensor of every launch of the three configurations of
tests/geometry_classes.py at B in {1, 37, 256} of 256 with producer and consumer agreeing, and the scan."""
import pytest

import host_build
from poserisk_release_amd import synth, weights


@pytest.fixture(scope="module")
def native_run(tmp_path_factory):
    d = tmp_path_factory.mktemp("fence_check")
    exe = host_build.build(d, "fence_check", "fence_check.cc", sources=("host_plan.cc",), strict=True, without_compiler="skip")
    weights.flatten_state_dict(synth.hmr_state_dict(seed=1)).tofile(str(d / "blob.f32"))
    return exe.run(d / "blob.f32")


def test_guards_tail_offsets_and_scan_are_clean_under_asan_and_ubsan(native_run):
    last = native_run.stdout.strip().splitlines()[-1]
    assert last.startswith("fence_check: ") and last.endswith(" 0 failures"), last
    # 4 plans x 3 batch sizes x more than 100 tensors a plan (about 50 launches, two to four tensors each)
    assert int(last.split()[1]) > 4 * 3 * 100
