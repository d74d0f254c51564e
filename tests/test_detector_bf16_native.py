"""pr_det_fold_pack_bf16 (csrc/det_host.cc) under ASan + UBSan, as a stand-alone program with
its own main (tests/native/det_pack_bf16_check.cc; nothing sanitised is loaded into Python): the rounding rule's edge cases,
the refusals by name, the byte offsets, the bf16 activation plan, and the fold of truncated tables into an exact-size,
byte-aligned heap block, compared bit for bit with the numpy restatement (tests/det_bf16_ref.py)."""
import numpy as np
import pytest

import det_bf16_ref
import host_build
from poserisk_release_amd import detector

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
    return host_build.build(tmp_path_factory.mktemp("det_pack_bf16"), "det_pack_bf16_check", "det_pack_bf16_check.cc",
                            sources=("det_host.cc",), strict=True, without_compiler="skip")


@pytest.mark.parametrize("n_layers", (1, 2, 5, 12))
def test_the_bf16_pack_is_clean_under_sanitizers_and_equals_numpy(exe, tmp_path, n_layers):
    layers = detector.yolo_layers()[:n_layers]
    body = special_body(layers, n_layers)
    body.tofile(str(tmp_path / "body.f32"))
    r = exe.run(n_layers, tmp_path / "body.f32", repr(EPS), tmp_path / "packed.bin")
    assert r.stdout.strip().splitlines()[-1].endswith(" 0 failures")
    want, used = det_bf16_ref.numpy_fold_pack_bf16(body, layers, EPS)
    got = np.fromfile(str(tmp_path / "packed.bin"), np.uint8)
    assert used == body.size and got.size == want.size
    assert np.array_equal(got, want), f"{int((got != want).sum())} of {got.size} packed bytes differ"
