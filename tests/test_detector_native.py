"""The device-free half of the person detector (csrc/det_host.cc) under AddressSanitizer + UndefinedBehaviorSanitizer, as a
stand-alone program with its own main (tests/native/det_host_check.cc; nothing sanitised is loaded into Python): topology,
refusals, fold + pack of a truncated table compared with a numpy float64 restatement, and the activation-buffer plan walked
symbolically at several input sizes."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import det_ref
from conftest import REPO
from poserisk_release_amd import detector

CSRC = os.path.join(REPO, "poserisk_release_amd", "csrc")
N_LAYERS = 12          # layers 0..11: seven BatchNorm convolutions up to 128 channels, three shortcuts; 0.32 M floats
EPS = 1e-5


@pytest.fixture(scope="module")
def native_run(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    d = tmp_path_factory.mktemp("det_host")
    exe = str(d / "det_host_check")
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
           "-Wall", "-Werror", "-o", exe, os.path.join(REPO, "tests", "native", "det_host_check.cc"), os.path.join(CSRC, "det_host.cc")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    layers = detector.yolo_layers()[:N_LAYERS]
    rng = np.random.default_rng(4)
    body = rng.normal(0, 1, detector.weight_floats(layers)).astype(np.float32)
    p = 0
    for l in layers:                                  # running variances must be positive
        if l["type"] == detector.CONV:
            body[p + 3 * l["cout"]:p + 4 * l["cout"]] = rng.uniform(0.5, 1.5, l["cout"])
            p += 4 * l["cout"] + l["cout"] * l["cin"] * l["ksize"] ** 2
    body.tofile(str(d / "body.f32"))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, str(N_LAYERS), str(d / "body.f32"), repr(EPS), str(d / "packed.f32")], capture_output=True, text=True,
                       timeout=600, env=env)
    return r, body, layers, str(d / "packed.f32")


def test_det_host_is_clean_under_asan_and_ubsan(native_run):
    r = native_run[0]
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-6000:])
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr and "CHECK FAILED" not in r.stderr, r.stderr[-6000:]
    assert r.stdout.strip().splitlines()[-1].endswith(" 0 failures")


def test_fold_and_pack_of_a_truncated_table_equal_numpy_float64(native_run):
    r, body, layers, packed_path = native_run
    assert r.returncode == 0, r.stderr[-4000:]
    want, used = det_ref.numpy_fold_pack(body, layers, EPS)
    assert used == body.size
    got = np.fromfile(packed_path, np.float32)
    assert got.size == want.size
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), f"{int((got != want).sum())} of {got.size} packed floats differ"
