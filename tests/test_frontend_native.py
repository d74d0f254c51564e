"""The frame downscale's two halves on the CPU, under ASan + UBSan.

`csrc/resize_host.cc` (pr_resize_plan) and `csrc/resize.hip` (the kernel, compiled unchanged for the host against
tests/native/host_shim.h: a launch = nested loops over workgroups and threads) are built by g++ into one stand-alone driver,
tests/native/resize_native.cc, which runs every call in exact-size heap blocks.  Checked here, without a GPU: tables, mode and
every output byte against tests/resize_ref.py at every size pair, three frames a call, the output starting at every alignment."""
import numpy as np
import pytest

import host_build
import resize_ref as rr


@pytest.fixture(scope="module")
def native(tmp_path_factory):
    d = tmp_path_factory.mktemp("resize_native")
    exe = host_build.build(d, "resize_native", "resize_native.cc", stage=("resize.hip", "resize_host.cc"), shim=True)

    def run(*args):
        r = exe.run(*args)
        return r.stdout, r.stderr

    def resize(frames, h, w):
        """-> (mode, xofs, xcoef, yofs, ycoef, [dst u8[F,h,w,3] for the output at alignment 0, 1, 2, 3])"""
        frames = np.ascontiguousarray(frames, np.uint8)
        F, H, W, _ = frames.shape
        with open(d / "in.bin", "wb") as f:
            f.write(np.array([F, H, W, h, w], np.int32).tobytes() + frames.tobytes())
        run("resize", d / "in.bin", d / "out.bin")
        take = host_build.taker(d / "out.bin")
        mode = int(take(np.int32, 1)[0])
        tables = take(np.int32, w), take(np.int16, 2 * w), take(np.int32, h), take(np.int16, 2 * h)
        outs = [take(np.uint8, F * h * w * 3).reshape(F, h, w, 3) for _ in range(4)]
        take.done()
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
