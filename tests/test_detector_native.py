"""The device-free half of the person detector (csrc/det_host.cc) under ASan + UBSan, as a
stand-alone program with its own main (tests/native/det_host_check.cc; nothing sanitised is loaded into Python): topology,
refusals, fold + pack of a truncated table compared with a numpy float64 restatement, and the activation-buffer plan walked
symbolically at several input sizes."""
import numpy as np
import pytest

import det_ref
import host_build
from poserisk_release_amd import detector

N_LAYERS = 12          # layers 0..11: seven BatchNorm convolutions up to 128 channels, three shortcuts; 0.32 M floats
EPS = 1e-5


@pytest.fixture(scope="module")
def native_run(tmp_path_factory):
    d = tmp_path_factory.mktemp("det_host")
    exe = host_build.build(d, "det_host_check", "det_host_check.cc", sources=("det_host.cc",), strict=True, without_compiler="skip")
    layers = detector.yolo_layers()[:N_LAYERS]
    rng = np.random.default_rng(4)
    body = rng.normal(0, 1, detector.weight_floats(layers)).astype(np.float32)
    p = 0
    for l in layers:                                  # running variances must be positive
        if l["type"] == detector.CONV:
            body[p + 3 * l["cout"]:p + 4 * l["cout"]] = rng.uniform(0.5, 1.5, l["cout"])
            p += 4 * l["cout"] + l["cout"] * l["cin"] * l["ksize"] ** 2
    body.tofile(str(d / "body.f32"))
    r = exe.run(N_LAYERS, d / "body.f32", repr(EPS), d / "packed.f32")          # checked: every test stands on a clean run
    return r, body, layers, str(d / "packed.f32")


def test_det_host_is_clean_under_asan_and_ubsan(native_run):
    r = native_run[0]
    assert r.stdout.strip().splitlines()[-1].endswith(" 0 failures")


def test_fold_and_pack_of_a_truncated_table_equal_numpy_float64(native_run):
    _, body, layers, packed_path = native_run
    want, used = det_ref.numpy_fold_pack(body, layers, EPS)
    assert used == body.size
    got = np.fromfile(packed_path, np.float32)
    assert got.size == want.size
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), f"{int((got != want).sum())} of {got.size} packed floats differ"
