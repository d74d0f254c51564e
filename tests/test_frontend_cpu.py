"""The video front end without a GPU: the reference's size rule, pr_resize_plan against tests/resize_ref.py, the resize contract
against the float64 bilinear, mjpeg.AviReader on AviWriter's files, on a hand-built foreign layout and on everything it must
refuse, and the splice of the standard Huffman tables into frames that bring none."""
import ctypes as C
import os
import re
import struct

import numpy as np
import pytest

import avi_cases as ac
import jpeg_ref
import resize_ref as rr
from conftest import REPO
from poserisk_release_amd import _lib, frontend, jpeg, mjpeg

PAIR_IDS = [f"{W}x{H}-{w}x{h}" for (H, W), (h, w) in rr.PAIRS]


@pytest.mark.parametrize("size, want", [((1920, 1080), (800, 450)), ((1280, 720), (800, 450)), ((640, 480), (600, 450)),
                                        ((800, 450), (800, 450)), ((1080, 1920), (800, 1422)), ((801, 300), (800, 299)),
                                        ((700, 451), (698, 450))])
def test_target_size_is_the_reference_rule(size, want):
    assert frontend.target_size(*size) == want == rr.target_size(*size)


def test_target_size_arms_can_be_switched_off():
    assert frontend.target_size(1920, 1080, max_w=0) == (800, 450)            # the height arm alone: 1920 * 450 / 1080
    assert frontend.target_size(1920, 1080, max_h=0) == (800, 450)
    assert frontend.target_size(1080, 1920, max_w=0) == (253, 450)
    assert frontend.target_size(1920, 1080, max_w=0, max_h=0) == (1920, 1080)
    assert frontend.target_size(640, 480, max_h=0) == (640, 480)


@pytest.mark.parametrize("pair", rr.PAIRS, ids=PAIR_IDS)
def test_plan_tables_and_mode_equal_the_reference(pair):
    (H, W), (h, w) = pair
    got, want = frontend.resize_plan(H, W, h, w), rr.plan(H, W, h, w)
    for g, r, name in zip(got[:4], want[:4], ("xofs", "xcoef", "yofs", "ycoef")):
        assert g.dtype == r.dtype and np.array_equal(g, r), name
    assert got[4] == want[4]
    for ofs, coef, S in ((got[0], got[1], W), (got[2], got[3], H)):
        assert ofs.min() >= 0 and ofs.max() <= S - 1
        assert (coef.reshape(-1, 2).astype(np.int32).sum(1) == 2048).all() and coef.min() >= 0


def test_the_pairs_reach_what_they_are_there_for():
    assert [rr.mode(H, W, h, w) for (H, W), (h, w) in rr.PAIRS] == [2, 2, 2, 2, 0, 1, 2]
    up = rr.positions(31, 70)
    assert up[0] < 0 and np.floor(up[-1]) >= 30                                # the upscale reaches both clamps
    assert all(rr.positions(S, d)[0] >= 0 for (H, W), (h, w) in rr.PAIRS[:3] for S, d in ((W, w), (H, h)))


def test_plan_refusals_come_back_by_name():
    lib = _lib.load()
    a32, a16 = np.zeros(8, np.int32), np.zeros(16, np.int16)
    mode = np.full(1, -1, np.int32)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    good = [16, 16, 8, 8, ptr(a32), ptr(a16), ptr(a32), ptr(a16), ptr(mode)]
    for pos, value, word in ((0, 0, "every side must lie in 1..4096"), (1, 4097, "every side"), (2, 0, "every side"), (3, 4097, "every side"),
                             (4, None, "null xofs_host"), (5, None, "null xcoef_host"), (6, None, "null yofs_host"),
                             (7, None, "null ycoef_host"), (8, None, "null mode_host")):
        args = list(good)
        args[pos] = value
        assert lib.pr_resize_plan(*args) == -1, (pos, value)
        assert word in lib.pr_last_error().decode(), (pos, lib.pr_last_error())
    assert mode[0] == -1
    with pytest.raises(_lib.PoseRiskHipError, match="every side must lie"):
        frontend.resize_plan(5000, 16, 8, 8)
    assert lib.pr_resize_plan(4096, 1, 1, 4096, *[ptr(np.zeros(8192, np.int32)) for _ in range(4)], ptr(mode)) == 0


@pytest.mark.parametrize("pair", rr.PAIRS, ids=PAIR_IDS)
def test_the_contract_stays_within_one_level_of_the_float64_bilinear(pair):
    """The integer passes truncate twice and round once; measured maximum over these cases 0.83 levels."""
    (H, W), (h, w) = pair
    c = rr.contents(H, W, seed=7)
    worst = 0.0
    for name in ("noise", "white", "checker"):
        got = rr.linear(c[name], h, w).astype(np.float64)                      # the two passes, whatever the mode of the pair
        worst = max(worst, float(np.abs(got - rr.bilinear_f64(c[name], h, w)).max()))
    print(f"[contract] {W}x{H} -> {w}x{h}: max |integer - float64| = {worst:.3f} levels")
    assert worst < 1.0


def test_the_half_rule_is_the_rounded_mean_and_the_copy_a_copy():
    c = rr.contents(90, 160, seed=1)["noise"]
    half = rr.resize(c, 45, 80)
    mean = c.reshape(45, 2, 80, 2, 3).astype(np.float64).mean((1, 3))
    assert np.array_equal(half, np.floor(mean + 0.5).astype(np.uint8))
    assert np.array_equal(rr.resize(c, 90, 160), c)
    assert not np.array_equal(rr.resize(rr.contents(90, 161, seed=1)["noise"], 45, 80), half)


# ---- the container ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def clip():
    px = ac.clip_pixels()
    return px, ac.clip_frames(px)


def test_round_trip_through_the_writer_with_odd_frames_and_continuation_files(clip, tmp_path):
    _, frames = clip
    frames = [f + b"\0" * ((len(f) + i) & 1) for i, f in enumerate(frames)]      # odd and even lengths in turn
    assert {len(f) & 1 for f in frames} == {0, 1}
    with mjpeg.AviWriter(str(tmp_path / "one.avi"), 100, 48, 29.97) as w:
        for f in frames:
            w.write(f)
    r = mjpeg.AviReader(str(tmp_path / "one.avi"))
    assert r.frames() == frames and r.n_frames == 12 and abs(r.fps - 29.97) < 1e-9 and r.paths == [str(tmp_path / "one.avi")]
    assert (r.header["width"], r.header["height"], r.header["strf_width"], r.header["strf_height"]) == (100, 48, 100, 48)
    with mjpeg.AviWriter(str(tmp_path / "split.avi"), 100, 48, 25, split_bytes=8192) as w:
        for f in frames:
            w.write(f)
    assert len(w.paths) >= 3
    r = mjpeg.AviReader(str(tmp_path / "split.avi"))
    assert r.paths == w.paths and r.frames() == frames and r.fps == 25.0
    # a continuation file named on its own is its own video
    assert mjpeg.AviReader(w.paths[1]).n_frames < 12


def test_a_foreign_layout_is_read_in_file_order(clip, tmp_path):
    _, frames = clip
    data, expected = ac.foreign_avi(frames, 100, 48)
    assert b"idx1" not in data and data.count(b"RIFF") == 2 and b"AVIX" in data and b"rec " in data and b"00wb" in data
    p = tmp_path / "foreign.avi"
    p.write_bytes(data)
    r = mjpeg.AviReader(str(p))
    assert r.n_frames == 13 and r.frames() == expected and r.frames()[2] is r.frames()[1]
    assert r.header["video_stream"] == 1 and r.fps == 25.0


def test_fps_falls_back_from_the_stream_header_to_avih_to_30(clip, tmp_path):
    _, frames = clip
    for kw, want in ((dict(rate=30000, scale=1001), 30000 / 1001), (dict(rate=0, scale=0, us_per_frame=20000), 50.0),
                     (dict(rate=0, scale=0, us_per_frame=0), 30.0)):
        (tmp_path / "f.avi").write_bytes(ac.plain_avi(frames[:2], 100, 48, **kw))
        assert mjpeg.AviReader(str(tmp_path / "f.avi")).fps == want


def test_handler_or_compression_may_name_the_codec_in_either_case(clip, tmp_path):
    _, frames = clip
    for kw in (dict(handler=b"mjpg", compression=b"MJPG"), dict(handler=b"\0\0\0\0", compression=b"mjpg"), dict(handler=b"MJPG", compression=b"\0\0\0\0")):
        (tmp_path / "f.avi").write_bytes(ac.plain_avi(frames[:3], 100, 48, **kw))
        assert mjpeg.AviReader(str(tmp_path / "f.avi")).frames() == frames[:3]


def test_everything_else_is_refused_with_the_name_and_the_reason(clip, tmp_path):
    _, frames = clip
    good = ac.plain_avi(frames[:4], 100, 48)
    avi1 = lambda pol: frames[0][:2] + b"\xff\xe0\x00\x10AVI1" + bytes([pol]) + b"\0" * 9 + frames[0][2:]
    leaves = bytearray(good)
    at = good.index(b"00dc") + 4
    leaves[at:at + 4] = struct.pack("<I", len(good))                           # the first frame claims more than its list holds
    cases = {
        "h264.avi": (ac.plain_avi(frames[:2], 100, 48, handler=b"H264", compression=b"H264"), r"b'H264'.*not Motion-JPEG"),
        "novideo.avi": (ac.plain_avi(frames[:2], 100, 48, fcc_type=b"auds"), "no video stream"),
        "notriff.avi": (b"\x00\x00\x00\x18ftypmp42" + b"\0" * 64, "not a RIFF AVI file"),
        "short.avi": (b"RIFF", "not a RIFF AVI file"),
        "leaves.avi": (bytes(leaves), r"chunk b'00dc' at offset \d+ .*leaves its parent LIST b'movi'"),
        "truncated.avi": (good[:len(good) * 2 // 3], r"leaves its parent.*truncated"),
        "twofields.avi": (ac.plain_avi([frames[0], frames[1] + frames[2]], 100, 48), r"frame 1: interlaced Motion-JPEG \(two SOI"),
        "polarity1.avi": (ac.plain_avi([avi1(1)], 100, 48), r"frame 0: interlaced Motion-JPEG \(AVI1 field polarity 1"),
        "polarity2.avi": (ac.plain_avi([frames[0], avi1(2)], 100, 48), r"frame 1: interlaced.*polarity 2"),
        "emptyfirst.avi": (ac.plain_avi([b"", frames[0]], 100, 48), r"frame 0: the first video chunk is empty"),
    }
    for name, (data, why) in cases.items():
        (tmp_path / name).write_bytes(data)
        with pytest.raises(ValueError, match=why) as e:
            mjpeg.AviReader(str(tmp_path / name))
        assert name in str(e.value), name
    # AVI1 with polarity 0 (progressive, what ffmpeg writes) is read, and a thumbnail's SOI inside an APP1 segment is no field
    thumb = frames[0][:2] + b"\xff\xe1" + struct.pack(">H", 2 + len(frames[1])) + frames[1] + frames[0][2:]
    (tmp_path / "ok.avi").write_bytes(ac.plain_avi([avi1(0), thumb], 100, 48))
    assert mjpeg.AviReader(str(tmp_path / "ok.avi")).frames() == [avi1(0), thumb]
    assert mjpeg.is_avi(str(tmp_path / "ok.avi")) and not mjpeg.is_avi(str(tmp_path / "notriff.avi")) and not mjpeg.is_avi(str(tmp_path / "absent.avi"))


# ---- frames without Huffman tables --------------------------------------------------------------------------------------------
def test_the_standard_tables_are_libjpegs_and_the_encoder_plans():
    data = ac.pillow_jpeg(ac.clip_pixels(1)[0])
    assert mjpeg.STD_DHT == ac.dht_bytes(data) and len(mjpeg.STD_DHT) == 432
    plan = jpeg.encode_plan(90, "4:2:0", 0, 48, 100)
    header = plan["header"][:plan["header_bytes"]].tobytes()
    at = header.index(b"\xff\xc4")
    assert header[at:at + 432] == mjpeg.STD_DHT and header[at + 432:at + 434] == b"\xff\xda"


def test_a_frame_without_tables_gets_them_in_front_of_its_sos(clip, tmp_path):
    px, frames = clip
    bare = [ac.strip_dht(f) for f in frames]
    assert all(len(f) - len(b) == 432 and b"\xff\xc4" not in b[:b.index(b"\xff\xda")] for f, b in zip(frames, bare))
    # the parser on its own still refuses such a stream
    _, _, _, pst, *_ = jpeg.parse([bare[0]])
    assert pst[0] != 0 and "table" in jpeg.refusal_name(pst[0]).lower()
    (tmp_path / "bare.avi").write_bytes(ac.plain_avi(bare, 100, 48))
    got = mjpeg.AviReader(str(tmp_path / "bare.avi")).frames()
    for i, (g, f) in enumerate(zip(got, frames)):
        sos, has_dht, _, _ = mjpeg.inspect_frame(g)
        assert has_dht and g[sos - 432:sos] == mjpeg.STD_DHT and len(g) == len(f), i
        _, _, _, pst, H, W, _ = jpeg.parse([g])
        assert pst[0] == 0 and (H, W) == (48, 100), i
        if i < 4:                                                              # one frame of each kind through the numpy decoder
            assert np.array_equal(jpeg_ref.decode(g), jpeg_ref.decode(f)), i
    # a frame that brings its tables is passed on untouched
    (tmp_path / "full.avi").write_bytes(ac.plain_avi(frames, 100, 48))
    assert mjpeg.AviReader(str(tmp_path / "full.avi")).frames() == frames


def test_chunk_rule_fits_max_bytes_and_is_at_least_one():
    per = 1080 * 1920 * 3 + jpeg.workspace_bytes(1, 1080, 1920)
    assert frontend.chunk_frames(1080, 1920, 16 << 30) == min(1024, (16 << 30) // per)
    assert frontend.chunk_frames(1080, 1920, 5 * per) == 5 and frontend.chunk_frames(1080, 1920, 5 * per - 1) == 4
    assert frontend.chunk_frames(1080, 1920, 1) == 1 and frontend.chunk_frames(48, 100, 16 << 30) == 1024


# ---- the ABI ------------------------------------------------------------------------------------------------------------------
def test_the_new_symbols_are_declared_and_bound_and_the_abi_stays_15():
    header = open(os.path.join(REPO, "include", "poserisk_hip.h")).read()
    lib = _lib.load()
    for name in ("pr_resize_plan", "pr_resize_frames"):
        assert re.search(r"\bint " + name + r"\(", header), name
        assert name in _lib.SIGNATURES and getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    assert lib.pr_abi_version() == 16 == _lib.ABI_VERSION
    assert "PR_RESIZE_COPY = 0, PR_RESIZE_HALF = 1, PR_RESIZE_LINEAR = 2" in header
    assert (frontend.MODE_COPY, frontend.MODE_HALF, frontend.MODE_LINEAR) == (rr.MODE_COPY, rr.MODE_HALF, rr.MODE_LINEAR) == (0, 1, 2)
