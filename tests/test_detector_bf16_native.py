"""pr_det_fold_pack_bf16 (csrc/det_host.cc) under AddressSanitizer + UndefinedBehaviorSanitizer, as a stand-alone program with
its own main (tests/native/det_pack_bf16_check.cc; nothing sanitised is loaded into Python): the rounding rule's edge cases,
the refusals by name, the byte offsets, the bf16 activation plan, and the fold of truncated tables into an exact-size,
byte-aligned heap block, compared bit for bit with the numpy restatement (tests/det_bf16_ref.py)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import det_bf16_ref
from conftest import REPO
from poserisk_release_amd import detector

CSRC = os.path.join(REPO, "poserisk_release_amd", "csrc")
EPS = 1e-5


def special_body(layers, seed):
    """A random darknet body for `layers` with positive variances and, in the weights of the LAST convolution, rounding ties in
    both directions, values one float off a tie, a NaN and a value past the largest bf16."""
    rng = np.random.default_rng(seed)
    body = rng.normal(0, 1, detector.weight_floats(layers)).astype(np.float32)
    p = 0
    for l in layers:
        if l["type"] == detector.CONV:
            if l["bn"]:
                body[p + 3 * l["cout"]:p + 4 * l["cout"]] = rng.uniform(0.5, 1.5, l["cout"])
            p += (4 if l["bn"] else 1) * l["cout"] + l["cout"] * l["cin"] * l["ksize"] ** 2
    special = np.array([0x3f808000, 0x3f818000, 0x3f808001, 0x3f817fff, 0xbf808000, 0xbf818000, 0x7fc00000, 0x7f7fffff, 0xff7fffff],
                       np.uint32).view(np.float32)
    body[-special.size:] = special
    return body


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    path = str(tmp_path_factory.mktemp("det_pack_bf16") / "det_pack_bf16_check")
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
           "-Wall", "-Werror", "-o", path, os.path.join(REPO, "tests", "native", "det_pack_bf16_check.cc"), os.path.join(CSRC, "det_host.cc")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    return path


@pytest.mark.parametrize("n_layers", (1, 2, 5, 12))
def test_the_bf16_pack_is_clean_under_sanitizers_and_equals_numpy(exe, tmp_path, n_layers):
    layers = detector.yolo_layers()[:n_layers]
    body = special_body(layers, n_layers)
    body.tofile(str(tmp_path / "body.f32"))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, str(n_layers), str(tmp_path / "body.f32"), repr(EPS), str(tmp_path / "packed.bin")], capture_output=True,
                       text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-6000:])
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr and "CHECK FAILED" not in r.stderr, r.stderr[-6000:]
    assert r.stdout.strip().splitlines()[-1].endswith(" 0 failures")
    want, used = det_bf16_ref.numpy_fold_pack_bf16(body, layers, EPS)
    got = np.fromfile(str(tmp_path / "packed.bin"), np.uint8)
    assert used == body.size and got.size == want.size
    assert np.array_equal(got, want), f"{int((got != want).sum())} of {got.size} packed bytes differ"
