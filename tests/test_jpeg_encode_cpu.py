"""The JPEG encoder without a GPU: the numpy restatement of the contract (tests/jpeg_enc_ref.py) against Pillow's files, the
library's host half (pr_jpeg_encode_plan, pr_jpeg_encode_bound) against the restatement, and the Motion-JPEG AVI writer against
an independent RIFF reader (tests/riff_reader.py)."""
import hashlib

import numpy as np
import pytest

import jpeg_enc_cases as ec
import jpeg_enc_ref as er
import jpeg_ref as jr
import riff_reader
from poserisk_release_amd import jpeg, mjpeg


def test_the_reference_reproduces_every_golden_file():
    cases = ec.small_cases() + [ec.canvas_case()]
    names = [c["name"].split("_") for c in cases]
    for W, H in ((33, 17), (37, 29)):                       # every value of every axis with both odd-sized images
        mine = [n for n in names if n[0] == f"{W}x{H}"]
        assert {n[1] for n in mine} == {"smooth", "noise"} and {n[2] for n in mine} == {"444", "422", "420"}
        assert {n[3] for n in mine} == {"q1", "q30", "q75", "q90", "q100"} and {n[4] for n in mine} == {"none", "row", "b3"}
    assert {n[0] for n in names} == {"17x16", "33x17", "37x29", "48x32", "160x120", "1000x50", "1000x450"}
    assert "160x120_noise_420_q100_none" in {c["name"] for c in cases}
    for c in cases:
        got = er.encode(c["src"], c["quality"], c["subsampling"], c["restart_interval"])
        assert got == c["data"], c["name"]
        if c["src"].shape[0] < 100:
            assert er.encode(c["src"][..., ::-1], c["quality"], c["subsampling"], c["restart_interval"], bgr=True) == got


def test_the_files_decode_to_the_pixels_pillow_decodes():
    cases = [c for c in ec.small_cases() if c["src"].shape[0] * c["src"].shape[1] <= 160 * 120]
    assert len(cases) >= 40
    for c in cases:
        px = jr.decode(er.encode(c["src"], c["quality"], c["subsampling"], c["restart_interval"]))
        assert px.shape == c["src"].shape
        assert hashlib.sha256(np.ascontiguousarray(px).tobytes()).hexdigest() == c["px_sha256"], c["name"]


def test_the_plan_equals_the_reference_for_every_quality():
    for i, quality in enumerate(range(1, 101)):
        samp = ("4:4:4", "4:2:2", "4:2:0")[i % 3]
        ri = (0, -1, 3, 70000)[i % 4]
        H, W = 17 + i, 33 + 2 * i
        plan = jpeg.encode_plan(quality, samp, ri, H, W)
        hs, vs = er.SAMPLING[samp]
        want = er.header(H, W, quality, hs, vs, ri)
        assert plan["header_bytes"] == len(want) and plan["header"][:len(want)].tobytes() == want and not plan["header"][len(want):].any()
        qt = er.quant_tables(quality)
        np.testing.assert_array_equal(plan["quant"], qt)
        np.testing.assert_array_equal(plan["recip"].astype(np.int64), -(-(1 << 32) // (8 * qt)))
        assert (plan["width"], plan["height"], plan["hs"], plan["vs"], plan["quality"]) == (W, H, hs, vs, quality)
        assert plan["restart_interval"] == er.geometry(H, W, hs, vs, ri)[2]
        for t in range(2):
            for codes, lens, bits, vals in ((plan["dc_code"][t], plan["dc_len"][t], er.DC_BITS[t], er.DC_VALS[t]),
                                            (plan["ac_code"][t], plan["ac_len"][t], er.AC_BITS[t], er.AC_VALS[t])):
                table = er.huff_codes(bits, vals)
                for sym in range(len(codes)):
                    assert (int(codes[sym]), int(lens[sym])) == table.get(sym, (0, 0)), (quality, t, sym)


def test_the_plan_refuses_what_the_encoder_does_not_accept():
    from poserisk_release_amd import _lib
    for bad in ((0, "4:2:0", 0, 64, 64), (101, "4:2:0", 0, 64, 64), (90, "4:2:0", -2, 64, 64), (90, "4:2:0", 0, 15, 64),
                (90, "4:2:0", 0, 64, 4097)):
        with pytest.raises(_lib.PoseRiskHipError):
            jpeg.encode_plan(*bad)
    with pytest.raises(ValueError, match="4:1:1"):
        jpeg.encode_plan(90, "4:1:1", 0, 64, 64)


def test_the_bound_holds_for_noise_at_quality_100():
    rng = np.random.default_rng(11)
    for samp in er.SAMPLING:
        for H, W, ri in ((29, 37, 0), (29, 37, 1), (48, 64, -1)):
            img = rng.integers(0, 2, (H, W, 3), dtype=np.uint8) * 255          # saturated noise: the largest coefficients
            n = len(er.encode(img, 100, samp, ri))
            bound = jpeg.encode_bound(H, W, samp, ri)
            assert bound == er.encode_bound(H, W, *er.SAMPLING[samp], ri) and n <= bound, (samp, H, W, ri, n, bound)
            assert n > H * W                                                      # the image is a hard one
    assert jpeg.encode_bound(15, 64) == 0
    for ask in (jpeg.encode_bound, jpeg.encode_workspace_bytes):
        with pytest.raises(ValueError, match="4:1:1"):
            ask(*((64, 64) if ask is jpeg.encode_bound else (1, 64, 64)), "4:1:1")
    # the slot that always fits follows the sampling: 4:4:4 holds more blocks than the default 4:2:0
    assert jpeg.encode_bound(64, 64, "4:4:4") > jpeg.encode_bound(64, 64, "4:2:2") > jpeg.encode_bound(64, 64)
    assert jpeg.encode_workspace_bytes(2, 64, 64) > 0 and jpeg.encode_workspace_bytes(2, 15, 64) == 0


def _frames(n, seed=3):
    rng = np.random.default_rng(seed)
    return [bytes([0xFF, 0xD8]) + rng.integers(0, 256, int(k), dtype=np.uint8).tobytes() + bytes([0xFF, 0xD9])
            for k in rng.integers(100, 900, n)]


def test_avi_writer_round_trips_through_an_independent_reader(tmp_path):
    frames = _frames(23)
    frames[4] = frames[4][:-3] + frames[4][-2:] if len(frames[4]) % 2 == 0 else frames[4]     # make sure both parities occur
    assert {len(f) & 1 for f in frames} == {0, 1}
    path = tmp_path / "a.avi"
    with mjpeg.AviWriter(path, 1000, 450, 29.97) as w:
        for f in frames:
            w.write(f)
    assert w.paths == [str(path)] and w.frames_written == 23
    got = riff_reader.read_avi(path)
    assert (got["width"], got["height"], got["bi_width"], got["bi_height"]) == (1000, 450, 1000, 450)
    assert got["count"] == got["stream_count"] == 23 and got["streams"] == 1 and got["has_index"]
    assert abs(got["fps"] - 29.97) < 1e-6 and abs(got["usec_per_frame"] - 1e6 / 29.97) <= 1
    assert (got["type"], got["handler"], got["compression"]) == (b"vids", b"MJPG", b"MJPG")
    assert got["frames"] == frames and got["odd_padded"]
    assert got["index"] == [(o, len(f)) for o, f in zip(got["offsets"], frames)]


def test_avi_writer_splits_at_split_bytes(tmp_path):
    frames = _frames(40, seed=4)
    w = mjpeg.AviWriter(tmp_path / "b.avi", 64, 48, 30, split_bytes=4096)
    for f in frames:
        w.write(f)
    paths = w.close()
    assert len(paths) >= 4 and paths[0].endswith("b.avi") and paths[1].endswith("b.001.avi") and paths[2].endswith("b.002.avi")
    back = []
    for p in paths:
        got = riff_reader.read_avi(p)
        assert got["count"] == got["stream_count"] == len(got["frames"]) == len(got["index"]) >= 1 and got["fps"] == 30
        assert len(open(p, "rb").read()) <= 4096
        back += got["frames"]
    assert back == frames
    with pytest.raises(ValueError, match="after close"):
        w.write(frames[0])
    with pytest.raises(ValueError, match="does not fit"):
        mjpeg.AviWriter(tmp_path / "c.avi", 64, 48, 30, split_bytes=4096).write(b"x" * 5000)
