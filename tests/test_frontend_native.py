"""The frame downscale's two halves on the CPU, under AddressSanitizer + UndefinedBehaviorSanitizer.

`csrc/resize_host.cc` (pr_resize_plan) and `csrc/resize.hip` (the kernel, compiled unchanged for the host against
tests/native/jpeg_host_shim.h: a launch = nested loops over workgroups and threads) are built by g++ into one stand-alone driver,
tests/native/resize_native.cc, which runs every call in exact-size heap blocks.  Checked here, without a GPU: tables, mode and
every output byte against tests/resize_ref.py at every size pair, three frames a call, the output starting at every alignment."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import resize_ref as rr
from conftest import REPO

CSRC = os.path.join(REPO, "poserisk_release_amd", "csrc")
NATIVE = os.path.join(REPO, "tests", "native")


@pytest.fixture(scope="module")
def native(tmp_path_factory):
    gxx = shutil.which("g++")
    assert gxx is not None, "g++ is needed to build the host form of csrc/resize_host.cc and csrc/resize.hip"
    d = tmp_path_factory.mktemp("resize_native")
    for src, dst in ((os.path.join(CSRC, "resize.hip"), "resize.hip"), (os.path.join(CSRC, "resize_host.cc"), "resize_host.cc"),
                     (os.path.join(NATIVE, "jpeg_host_shim.h"), "common.h"),
                     (os.path.join(NATIVE, "resize_native.cc"), "resize_native.cc")):
        shutil.copy(src, d / dst)
    exe = str(d / "resize_native")
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
           "-Wno-unknown-pragmas", "-x", "c++", "-I", str(d), "-I", CSRC, "-o", exe, str(d / "resize_native.cc")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")

    def run(*args):
        r = subprocess.run([exe, *[str(a) for a in args]], capture_output=True, text=True, timeout=600, env=env)
        assert r.returncode == 0 and "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, (r.returncode, r.stderr[-6000:])
        return r.stdout, r.stderr

    def resize(frames, h, w):
        """-> (mode, xofs, xcoef, yofs, ycoef, [dst u8[F,h,w,3] for the output at alignment 0, 1, 2, 3])"""
        frames = np.ascontiguousarray(frames, np.uint8)
        F, H, W, _ = frames.shape
        with open(d / "in.bin", "wb") as f:
            f.write(np.array([F, H, W, h, w], np.int32).tobytes() + frames.tobytes())
        run("resize", d / "in.bin", d / "out.bin")
        raw, pos = np.fromfile(d / "out.bin", np.uint8), 0

        def take(dtype, n):
            nonlocal pos
            a = raw[pos:pos + n * np.dtype(dtype).itemsize].view(dtype)
            pos += a.nbytes
            return a
        mode = int(take(np.int32, 1)[0])
        tables = take(np.int32, w), take(np.int16, 2 * w), take(np.int32, h), take(np.int16, 2 * h)
        outs = [take(np.uint8, F * h * w * 3).reshape(F, h, w, 3) for _ in range(4)]
        assert pos == raw.size
        return (mode, *tables, outs)
    return run, resize


@pytest.mark.parametrize("pair", rr.PAIRS, ids=lambda p: f"{p[0][1]}x{p[0][0]}-{p[1][1]}x{p[1][0]}")
def test_three_frames_at_every_alignment_equal_the_reference(native, pair):
    _, resize = native
    (H, W), (h, w) = pair
    c = rr.contents(H, W, seed=H + W)
    frames = np.stack([c["noise"], c["checker"], c["gradient"]])
    mode, xofs, xcoef, yofs, ycoef, outs = resize(frames, h, w)
    want = rr.plan(H, W, h, w)
    assert mode == want[4]
    for got, ref, name in zip((xofs, xcoef, yofs, ycoef), want, ("xofs", "xcoef", "yofs", "ycoef")):
        assert np.array_equal(got, ref), name
    ref = rr.resize(frames, h, w)
    for shift, got in enumerate(outs):
        bad = np.argwhere(got != ref)
        assert bad.size == 0, f"alignment {shift}: {len(bad)} bytes differ, first (frame, row, col, channel) {bad[0].tolist()}"


def test_the_odd_pair_starts_its_later_frames_unaligned():
    (_, _), (h, w) = rr.PAIRS[2]
    assert h * w * 3 == 1173 and {(k * 1173) % 4 for k in range(3)} == {0, 1, 2}


def test_every_argument_error_is_refused_by_name(native):
    run, _ = native
    out, err = run("refusals")
    assert "18 of 18 bad calls refused" in out
    for word in ("null xofs_host", "null mode_host", "every side must lie in 1..4096", "null src", "null ycoef", "mode = 2", "F = -1"):
        assert word in err, word
