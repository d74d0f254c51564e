"""The YUV4MPEG2 writer's two halves on the CPU, under ASan + UBSan.

`csrc/y4m_host.cc` (the forward matrix's integers, and the FRAME index that reads the result back) and `csrc/yuv_enc.hip` (the
kernel, compiled unchanged for the host against tests/native/host_shim.h: a launch = nested loops over workgroups and
threads) are built by g++ into one stand-alone driver, tests/native/yuv_enc_native.cc, which runs every call in exact-size heap
blocks.  Checked here, without a GPU: every output byte against tests/yuv_enc_ref.py for every chroma layout, six sizes, three
frames a call (so frames begin at different alignments), both matrices and ranges, bgr, padding 0 and 1 on each axis, and src and
dst starting at each of the four byte alignments."""
import numpy as np
import pytest

import host_build
import yuv_enc_ref as er

MATRIX = {"601": 0, "709": 1}
SIZES = ((1, 1), (2, 2), (3, 3), (7, 5), (17, 13), (64, 2))            # (W, H)
F = 3


@pytest.fixture(scope="module")
def native(tmp_path_factory):
    d = tmp_path_factory.mktemp("yuv_enc_native")
    exe = host_build.build(d, "yuv_enc_native", "yuv_enc_native.cc", stage=("yuv_enc.hip", "y4m_host.cc"), shim=True)

    def run(*args):
        r = exe.run(*args)
        return r.stdout, r.stderr

    def encode(calls):
        """calls: [(frames u8[F,H,W,3], chroma, matrix, full_range, bgr, (out_H, out_W))] -> [(plan, [bytes at dst alignment
        0, 1, 2, 3])]"""
        blob = bytearray(np.array([len(calls)], np.int32).tobytes())
        for frames, chroma, matrix, full, bgr, (oh, ow) in calls:
            n, H, W, _ = frames.shape
            blob += np.array([MATRIX[matrix], int(full), int(bgr), er.CHROMAS.index(chroma), n, H, W, oh, ow], np.int32).tobytes()
            blob += np.ascontiguousarray(frames).tobytes()
        (d / "in.bin").write_bytes(bytes(blob))
        run("encode", d / "in.bin", d / "out.bin")
        raw, pos, results = (d / "out.bin").read_bytes(), 0, []
        for _ in calls:
            total = int(np.frombuffer(raw, np.int32, 1, pos)[0])
            plan = tuple(np.frombuffer(raw, np.int32, 9, pos + 4).tolist())
            pos += 40
            results.append((plan, [raw[pos + k * total:pos + (k + 1) * total] for k in range(4)]))
            pos += 4 * total
        assert pos == len(raw)
        return results
    return run, encode


def _first_difference(got, want):
    got, want = np.frombuffer(got, np.uint8), np.frombuffer(want, np.uint8)
    if got.size != want.size:
        return f"{got.size} bytes for {want.size}"
    bad = np.nonzero(got != want)[0]
    return f"{bad.size} bytes differ, first at byte {bad[0]}: {got[bad[0]]} for {want[bad[0]]}"


@pytest.mark.parametrize("chroma", er.CHROMAS)
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_every_layout_matrix_range_order_and_padding_equals_the_reference(native, chroma, size):
    _, encode = native
    W, H = size
    frames = np.random.default_rng(W * 100 + H).integers(0, 256, (F, H, W, 3), dtype=np.uint8)
    calls = []
    for pad_h in (0, 1):
        for pad_w in (0, 1):
            for matrix in ("601", "709"):
                for full in (False, True):
                    for bgr in (False, True) if (matrix, full) == ("601", False) else (False,):
                        calls.append((frames, chroma, matrix, full, bgr, (H + pad_h, W + pad_w)))
    for (frames, chroma, matrix, full, bgr, out), (plan, outs) in zip(calls, encode(calls)):
        assert plan == er.plan(matrix, full)
        want = er.encode(frames, chroma, matrix, full, bgr, out)
        assert len(want) == F * (6 + er.frame_bytes(out[1], out[0], chroma))
        for shift, got in enumerate(outs):
            assert got == want, (f"{chroma} {matrix} full={full} bgr={bgr} padded to {out[1]}x{out[0]}, dst at alignment {shift}: "
                                 + _first_difference(got, want))


@pytest.mark.parametrize("chroma", er.CHROMAS)
def test_extreme_colours(native, chroma):
    """Primaries, black and white, and 0 / 255 noise: where chroma would leave the byte range without its clamp."""
    _, encode = native
    rng = np.random.default_rng(2)
    flat = np.array([[255, 0, 0], [0, 255, 0], [0, 0, 255], [0, 0, 0], [255, 255, 255]], np.uint8)
    frames = np.concatenate([np.broadcast_to(flat[:, None, None, :], (5, 5, 7, 3)),
                             (255 * rng.integers(0, 2, (2, 5, 7, 3))).astype(np.uint8)])
    calls = [(frames, chroma, m, full, False, (6, 8)) for m in ("601", "709") for full in (False, True)]
    for (frames, chroma, matrix, full, bgr, out), (_, outs) in zip(calls, encode(calls)):
        want = er.encode(frames, chroma, matrix, full, bgr, out)
        assert all(got == want for got in outs), (matrix, full, _first_difference(outs[0], want))


def test_every_argument_error_is_refused_by_name(native):
    run, _ = native
    out, err = run("refusals")
    assert "18 of 18 bad calls refused" in out
    for word in ("matrix = 2", "matrix = -1", "full_range = 2", "full_range = -1", "null plan_host", "null args", "F = -1",
                 "every side must lie in 1..4096", "the padded picture", "a side grows by 0 or 1", "chroma = 5", "chroma = -1", "null src",
                 "null dst"):
        assert word in err, word
