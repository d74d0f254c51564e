"""The YUV4MPEG2 reader's two halves on the CPU, under ASan + UBSan.

`csrc/y4m_host.cc` (header, FRAME index, matrix integers) and `csrc/yuv.hip` (the kernel, compiled unchanged for the host
against tests/native/host_shim.h: a launch = nested loops over workgroups and threads) are built by g++ into one stand-alone
driver, tests/native/y4m_native.cc, which runs every call in exact-size heap blocks.  Checked here, without a GPU: every output
byte against tests/yuv_ref.py (and tests/resize_ref.py for the fused downscale) for every chroma layout, both matrices and
ranges, bgr, seven sizes, frame payloads at all four byte alignments and the output starting at every alignment."""
import numpy as np
import pytest

import host_build
import resize_ref as rr
import y4m_cases as yc
import yuv_ref

MATRIX = {"601": 0, "709": 1}


@pytest.fixture(scope="module")
def native(tmp_path_factory):
    d = tmp_path_factory.mktemp("y4m_native")
    exe = host_build.build(d, "y4m_native", "y4m_native.cc", stage=("yuv.hip", "y4m_host.cc", "resize_host.cc"), shim=True)

    def run(*args):
        r = exe.run(*args)
        return r.stdout, r.stderr

    def frames(data, matrix="601", full_range=None, bgr=False, size=None):
        """-> (head dict, plan, offsets, [dst u8[F,h,w,3] for the output at alignment 0, 1, 2, 3])"""
        h, w = size or (0, 0)
        with open(d / "in.bin", "wb") as f:
            f.write(np.array([MATRIX[matrix], -1 if full_range is None else int(full_range), int(bgr), h, w, len(data)], np.int32).tobytes()
                    + data)
        run("frames", d / "in.bin", d / "out.bin")
        take = host_build.taker(d / "out.bin")
        names = ("F", "H", "W", "chroma", "full_range", "fps_num", "fps_den", "header_bytes", "h", "w", "mode")
        head = dict(zip(names, take(np.int32, 11).tolist()))
        plan = tuple(take(np.int32, 6).tolist())
        offsets = take(np.int64, head["F"]).tolist()
        outs = [take(np.uint8, head["F"] * head["h"] * head["w"] * 3).reshape(head["F"], head["h"], head["w"], 3) for _ in range(4)]
        take.done()
        return head, plan, offsets, outs
    return run, frames


def _check(outs, want, what):
    for shift, got in enumerate(outs):
        bad = np.argwhere(got != want)
        assert bad.size == 0, (f"{what}, output at alignment {shift}: {len(bad)} bytes differ, first (frame, row, col, channel) "
                               f"{bad[0].tolist()}: {got[tuple(bad[0])]} for {want[tuple(bad[0])]}")


@pytest.mark.parametrize("chroma", yuv_ref.CHROMAS)
@pytest.mark.parametrize("size", yc.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_every_layout_matrix_range_and_order_equals_the_reference(native, chroma, size):
    """Five frames a call, their payloads at byte alignments 0, 1, 2, 3, 0 of the chunk."""
    _, frames = native
    W, H = size
    data, offsets, (Y, U, V) = yc.case(W, H, chroma, F=5, seed=W * 100 + H)
    assert yc.alignments(offsets) == {0, 1, 2, 3}
    for matrix in ("601", "709"):
        for full in (False, True):
            for bgr in (False, True) if (matrix, full) == ("601", False) else (False,):
                head, plan, got_offsets, outs = frames(data, matrix, full, bgr)
                assert (head["F"], head["H"], head["W"], yuv_ref.CHROMAS[head["chroma"]]) == (5, H, W, chroma)
                assert (head["fps_num"], head["fps_den"], head["full_range"], head["mode"]) == (25, 1, -1, 0)
                assert got_offsets == offsets and plan == yuv_ref.plan(matrix, full)
                _check(outs, yuv_ref.convert(Y, U, V, chroma, matrix, full, bgr), f"{chroma} {matrix} full={full} bgr={bgr}")


@pytest.mark.parametrize("chroma", yuv_ref.CHROMAS)
def test_extreme_samples_and_the_headers_own_range(native, chroma):
    _, frames = native
    data, _, (Y, U, V) = yc.case(7, 5, chroma, F=4, seed=3, colorrange="FULL", kind="extreme")
    head, plan, _, outs = frames(data, "709")
    assert head["full_range"] == 1 and plan == yuv_ref.plan("709", True)
    _check(outs, yuv_ref.convert(Y, U, V, chroma, "709", True), f"{chroma} extreme")


@pytest.mark.parametrize("chroma", yuv_ref.CHROMAS)
@pytest.mark.parametrize("pair", (((37, 53), (37, 53)), ((20, 32), (10, 16)), ((37, 53), (17, 23))), ids=("copy", "half", "linear"))
def test_the_fused_downscale_equals_convert_then_resize(native, chroma, pair):
    """COPY, HALF (32x20 -> 16x10) and LINEAR (53x37 -> 23x17, 1173 bytes a frame, so later frames start unaligned)."""
    _, frames = native
    (H, W), (h, w) = pair
    data, offsets, (Y, U, V) = yc.case(W, H, chroma, F=4, seed=H + w)
    assert yc.alignments(offsets) == {0, 1, 2, 3}
    for matrix, full, bgr in (("601", False, False), ("709", True, True)):
        head, _, _, outs = frames(data, matrix, full, bgr, size=(h, w))
        assert (head["h"], head["w"], head["mode"]) == (h, w, rr.mode(H, W, h, w))
        _check(outs, rr.resize(yuv_ref.convert(Y, U, V, chroma, matrix, full, bgr), h, w), f"{chroma} {W}x{H} -> {w}x{h}")


def test_every_argument_error_is_refused_by_name(native):
    run, _ = native
    out, err = run("refusals")
    assert "35 of 35 bad calls refused" in out
    for word in ("null data_host", "null info_host", "n = -1", "null offsets_host", "null n_frames_host", "null consumed_host",
                 "max_frames = -1", "info is not what pr_y4m_parse_header fills", "matrix = 2", "full_range = 2", "null plan_host",
                 "null args", "F = -1", "every side must lie in 1..4096", "chroma = 5", "data_bytes = -1", "null data", "null offsets",
                 "null dst", "no downscale", "mode = 2", "null xofs", "null xcoef", "null yofs", "null ycoef"):
        assert word in err, word
