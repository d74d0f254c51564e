"""The internal fence's device-free part under AddressSanitizer + UndefinedBehaviorSanitizer, on the CPU.

POSERISK_FENCE (DESIGN.md "The internal fence") puts every device allocation of the library's own between guards and, in tail
mode, ends every tensor of the encoder's workspaces on its buffer's last byte.  What decides that without a device -- the
guard size, the tail offset, the scan of a guard's host copy (csrc/host_common.h) and the byte sizes hmr.hip places each
tensor by (csrc/host_plan.h) -- is held here by a stand-alone program, tests/native/fence_check.cc (its header lists the
checks): guard sizes, the tail placement of every tensor of every launch of the three configurations of
tests/geometry_classes.py at B in {1, 37, 256} of 256 with producer and consumer agreeing, and the scan."""
import os
import shutil
import subprocess

import pytest

from conftest import REPO
from poserisk_release_amd import synth, weights


@pytest.fixture(scope="module")
def native_run(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    d = tmp_path_factory.mktemp("fence_check")
    exe = str(d / "fence_check")
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
           "-Wall", "-Werror", "-o", exe, os.path.join(REPO, "tests", "native", "fence_check.cc"),
           os.path.join(REPO, "poserisk_release_amd", "csrc", "host_plan.cc")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    weights.flatten_state_dict(synth.hmr_state_dict(seed=1)).tofile(str(d / "blob.f32"))
    env = {k: v for k, v in os.environ.items() if not k.startswith("POSERISK_")}
    env.update(ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    return subprocess.run([exe, str(d / "blob.f32")], capture_output=True, text=True, timeout=600, env=env)


def test_guards_tail_offsets_and_scan_are_clean_under_asan_and_ubsan(native_run):
    r = native_run
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-6000:])
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr and "CHECK FAILED" not in r.stderr, r.stderr[-6000:]
    last = r.stdout.strip().splitlines()[-1]
    assert last.startswith("fence_check: ") and last.endswith(" 0 failures"), last
    # 4 plans x 3 batch sizes x more than 100 tensors a plan (about 50 launches, two to four tensors each)
    assert int(last.split()[1]) > 4 * 3 * 100
