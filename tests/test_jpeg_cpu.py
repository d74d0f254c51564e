"""CPU-only checks of the JPEG decoder: the numpy restatement of the contract (tests/jpeg_ref.py) against libjpeg's pixels, the
host parser through the C ABI, the new entry points' refusals, and the ordering of a folder of frames."""
import ctypes as C
import io
import os
import re

import numpy as np
import pytest

import jpeg_cases as jc
import jpeg_ref as jr
from conftest import REPO
from poserisk_release_amd import _lib, jpeg


def test_reference_equals_every_small_golden_case():
    cases = jc.small_cases()
    assert len(cases) >= 36
    for name, stream, want in cases:
        got = jr.decode_strict(stream)
        bad = np.argwhere(got != want)
        assert bad.size == 0, f"{name}: {len(bad)} bytes differ, first (row, col, channel) {bad[0].tolist()}"
        assert np.array_equal(jr.decode(stream, bgr=True), want[..., ::-1]), name


def test_golden_frames_are_what_the_issue_names():
    fr = jc.frames_800x450()
    assert [n for n, *_ in fr] == ["420_q95", "420_q95_rstrow", "420_q95_opt", "444_q95"]
    for name, stream, sha, pos, val in fr:
        p = jr.parse(stream)
        assert (p["width"], p["height"]) == (800, 450) and len(sha) == 64 and pos.shape == val.shape == (4096,), name
        assert (p["hs"], p["vs"]) == ((1, 1) if name.startswith("444") else (2, 2)), name
        assert (p["restart"] > 0) == ("rstrow" in name) and len(p["segments"]) == (29 if "rstrow" in name else 1), name
    for f in ("jpeg_cases.npz", "jpeg_frames.npz"):
        assert os.path.getsize(os.path.join(jc.GOLDEN, f)) < 1 << 20


def test_reference_equals_live_pillow():
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(31)
    for k, (H, W, kw) in enumerate([(41, 23, dict(quality=77, subsampling=2)), (24, 56, dict(quality=93, subsampling=1, optimize=True)),
                                    (19, 35, dict(quality=100, subsampling=0, restart_marker_blocks=2)),
                                    (33, 33, dict(quality=40, subsampling=2, restart_marker_rows=1))]):
        img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8) if k % 2 else \
            np.clip(np.add.outer(np.arange(H) * 5, np.arange(W) * 3)[..., None] + rng.normal(0, 9, (H, W, 3)), 0, 255).astype(np.uint8)
        for gray in (False, True):
            buf = io.BytesIO()
            (Image.fromarray(img).convert("L") if gray else Image.fromarray(img)).save(buf, "JPEG", **kw)
            want = np.asarray(Image.open(io.BytesIO(buf.getvalue())).convert("RGB"))
            assert np.array_equal(jr.decode_strict(buf.getvalue()), want), (H, W, kw, gray)


def test_new_symbols_are_declared_bound_and_the_abi_stays_15():
    hdr = open(os.path.join(REPO, "include", "poserisk_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = _lib.load()
    for name in ("pr_jpeg_parse", "pr_jpeg_refusal_name", "pr_jpeg_workspace_bytes", "pr_jpeg_decode"):
        assert re.search(r"\b" + name + r"\s*\(", hdr) and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert lib.pr_abi_version() == _lib.ABI_VERSION == 16
    # the binding's records are the header's structs
    assert jpeg.FRAME_DTYPE.itemsize == 15 * 4 + 3 * 64 * 2 and jpeg.SEGMENT_DTYPE.itemsize == 24
    assert jpeg.HUFF_DTYPE.itemsize == 4 * (1024 + 68 + 68 + 256 + 4)
    assert C.sizeof(_lib.JpegArgs) == 6 * 8 + 8 + 6 * 4
    for code, word in ((jr.PROGRESSIVE, "progressive"), (jr.ARITHMETIC, "arithmetic"), (jr.PRECISION, "precision"),
                       (jr.COMPONENTS, "component"), (jr.SAMPLING, "sampling"), (jr.SCANS, "scan"), (jr.QUANT16, "16-bit"),
                       (jr.DIMENSIONS, "16..4096"), (jr.TRUNCATED, "truncated"), (jr.SIZE_DIFFERS, "size differs")):
        assert word in jpeg.refusal_name(code), (code, jpeg.refusal_name(code))


def test_the_library_parser_equals_the_reference_on_a_mixed_call():
    """Through ctypes as decode_files calls it: many files in one buffer, table sets stored once per distinct set."""
    cases = [c for c in jc.small_cases() if c[0].startswith("48x32")]
    blobs = [s for _, s, _ in cases] + [cases[0][1]]
    frames, segs, huff, pst, H, W, offsets = jpeg.parse(blobs)
    assert (H, W) == (32, 48) and not pst.any()
    n_seg = 0
    for f, blob in enumerate(blobs):
        p = jr.parse(blob)
        assert frames[f]["first_segment"] == n_seg and frames[f]["n_segments"] == len(p["segments"])
        mine = segs[n_seg:n_seg + len(p["segments"])]
        assert [(int(s["begin"] - offsets[f]), int(s["end"] - offsets[f]), int(s["first_mcu"]), int(s["frame"])) for s in mine] == \
            [(b, e, m, f) for b, e, m in p["segments"]]
        n_seg += len(p["segments"])
    assert n_seg == len(segs)
    # standard tables are one set for colour and one for gray (it uses two of the four tables); optimised ones are their own
    assert frames[-1]["huff_set"] == frames[0]["huff_set"] and len(huff) < len(blobs)
    assert len({int(f["huff_set"]) for f in frames}) == len(huff)


def _mutate(stream, marker, offset, value):
    i = stream.index(marker)
    return stream[:i + offset] + bytes([value]) + stream[i + offset + 1:]


def test_everything_outside_the_accepted_subset_is_refused_by_name():
    base = next(s for n, s, _ in jc.small_cases() if n == "48x32_420_q75")
    sof, sos, dqt = b"\xff\xc0", b"\xff\xda", b"\xff\xdb"
    bad = {
        jr.PROGRESSIVE: _mutate(base, sof, 1, 0xC2), jr.EXTENDED: _mutate(base, sof, 1, 0xC1), jr.ARITHMETIC: _mutate(base, sof, 1, 0xC9),
        jr.PRECISION: _mutate(base, sof, 4, 12), jr.COMPONENTS: _mutate(base, sof, 9, 4), jr.SAMPLING: _mutate(base, sof, 11, 0x12),
        jr.DIMENSIONS: _mutate(base, sof, 6, 15), jr.QUANT16: _mutate(base, dqt, 4, 0x10), jr.SCANS: _mutate(base, sos, 4, 1),
        jr.NOT_JPEG: b"\x89PNG" + base, jr.TRUNCATED: base[:-2], jr.TABLE: _mutate(base, sos, 6, 0x22),
    }
    bad[jr.DIMENSIONS] = _mutate(_mutate(base, sof, 5, 0), sof, 6, 15)      # height 15
    blobs = [base] + list(bad.values()) + [next(s for n, s, _ in jc.small_cases() if n == "33x17_420_q75")]
    frames, segs, huff, pst, H, W, _ = jpeg.parse(blobs)
    assert pst.tolist() == [0] + list(bad.keys()) + [jr.SIZE_DIFFERS]
    assert [jr.parse_status(b) for b in blobs[:-1]] == pst.tolist()[:-1]
    assert (frames["ncomp"][1:] == 0).all() and frames["ncomp"][0] == 3 and len(segs) == 1
    msg = _lib.load().pr_last_error().decode()
    assert "frame %d refused" % (len(blobs) - 1) in msg and "size differs" in msg


def test_the_size_of_a_call_comes_from_the_first_accepted_frame_not_the_first_parsed_header():
    """A frame whose header parses but which is refused later (its EOI cut off, a restart marker out of sequence) must not fix
    H x W: the good frames of another size behind it are the call's frames."""
    case = lambda n: next(s for m, s, _ in jc.small_cases() if m == n)
    big, small = case("48x32_420_q75"), case("33x17_420_q75")
    rst = case("48x32_420_q95_rstrow")
    i = rst.index(b"\xff\xd0")
    for damaged, why in ((big[:-2], jr.TRUNCATED), (rst[:i + 1] + b"\xd3" + rst[i + 2:], jr.RESTARTS)):
        frames, segs, huff, pst, H, W, _ = jpeg.parse([damaged, small, small, big])
        assert (H, W) == (17, 33) and pst.tolist() == [why, 0, 0, jr.SIZE_DIFFERS]
        assert frames["width"].tolist()[1:3] == [33, 33] and len(segs) == 2 and len(huff) == 1
    # with nothing accepted there is no size
    assert jpeg.parse([big[:-2], small[:-2]])[4:6] == (0, 0)


def test_null_pointers_sizes_and_workspace_are_refused_by_name_before_any_device_work():
    lib = _lib.load()
    err = lambda: lib.pr_last_error().decode()
    base = next(s for n, s, _ in jc.small_cases() if n == "48x32_420_q75")
    data = np.frombuffer(base, np.uint8)
    off = np.array([0, len(base)], np.int64)
    fr, seg, hf = np.zeros(1, jpeg.FRAME_DTYPE), np.zeros(4, jpeg.SEGMENT_DTYPE), np.zeros(1, jpeg.HUFF_DTYPE)
    st, counts = np.zeros(1, np.int32), np.zeros(4, np.int32)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    full = [ptr(data), ptr(off), 1, 0, 0, ptr(fr), ptr(seg), 4, ptr(hf), 1, ptr(st), ptr(counts)]
    assert lib.pr_jpeg_parse(*full) == 0 and counts.tolist() == [1, 1, 32, 48]
    for i, word in ((0, "null data_host"), (1, "null offsets_host"), (5, "null frames_host"), (6, "null segments_host"),
                    (8, "null huff_host"), (10, "null parse_status_host"), (11, "null counts_host")):
        args = list(full)
        args[i] = None
        assert lib.pr_jpeg_parse(*args) == -1 and word in err(), (i, err())
    assert lib.pr_jpeg_parse(*(full[:2] + [-1] + full[3:])) == -1 and "F = -1" in err()
    assert lib.pr_jpeg_parse(*(full[:3] + [8, 48] + full[5:])) == -1 and "8 x 48" in err()
    assert lib.pr_jpeg_parse(ptr(data), ptr(np.array([5, 2], np.int64)), *full[2:]) == -1 and "below" in err()
    assert lib.pr_jpeg_parse(*(full[:7] + [0] + full[8:])) == -4 and "1 segments" in err() and counts[0] == 1     # PR_ERR_CAPACITY
    assert lib.pr_jpeg_parse(None, None, 0, 0, 0, None, None, 0, None, 0, None, ptr(counts)) == 0                  # an empty batch
    assert lib.pr_jpeg_parse(*(full[:3] + [17, 33] + full[5:])) == 0 and st[0] == jr.SIZE_DIFFERS
    # pr_jpeg_decode: every refusal below comes before anything is launched or dereferenced (the pointers are not memory)
    assert lib.pr_jpeg_workspace_bytes(2, 450, 800) == 2 * 3 * 800 * 464 * 3 and lib.pr_jpeg_workspace_bytes(0, 16, 16) == 0
    fake = 0x1000
    def call(ws=fake, ws_bytes=1 << 40, **kw):
        f = dict(data=fake, frames=fake, segments=fake, huff=fake, out=fake, status=fake, data_bytes=100, F=1, H=32, W=48,
                 n_segments=1, n_huff=1, bgr=0)
        f.update(kw)
        return lib.pr_jpeg_decode(_lib.JpegArgs(**f), ws, ws_bytes, None)
    assert lib.pr_jpeg_decode(None, fake, 1, None) == -1 and "null argument struct" in err()
    assert call(F=0, frames=None, out=None, status=None, ws=None, ws_bytes=0) == 0                                 # an empty batch
    for kw, word in ((dict(frames=None), "null frames"), (dict(out=None), "null out"), (dict(status=None), "null status"),
                     (dict(data=None), "need data"), (dict(segments=None), "need data"), (dict(huff=None), "need data"),
                     (dict(n_huff=0), "n_huff = 0"), (dict(F=-2), "F = -2"), (dict(H=8), "8 x 48"), (dict(W=5000), "32 x 5000"),
                     (dict(n_segments=-1), "negative count"), (dict(ws=None), "null workspace"), (dict(ws=fake + 4), "16-byte"),
                     (dict(ws_bytes=lib.pr_jpeg_workspace_bytes(1, 32, 48) - 1), "needed for 1 frames of 32 x 48")):
        assert call(**kw) == -1 and word in err(), (kw, err())


def test_list_frames_orders_by_name_and_refuses_png(tmp_path):
    names = ["000000010.jpg", "000000002.JPG", "000000001.jpeg", "000000003.Jpeg", "b.jpg", "B.jpg", "tracking.pkl", "fps.txt",
             "frames.txt", "thumb.jpg.bak"]
    for n in names:
        (tmp_path / n).write_bytes(b"x")
    got = jpeg.list_frames(str(tmp_path))
    assert got == sorted(n for n in names if n.lower().endswith((".jpg", ".jpeg")))
    assert got[:4] == ["000000001.jpeg", "000000002.JPG", "000000003.Jpeg", "000000010.jpg"]
    (tmp_path / "000000004.PNG").write_bytes(b"x")
    with pytest.raises(ValueError, match=r"000000004\.PNG.*PNG frames are not supported"):
        jpeg.list_frames(str(tmp_path))
    (tmp_path / "empty").mkdir()
    assert jpeg.list_frames(str(tmp_path / "empty")) == []
    with pytest.raises(_lib.PoseRiskHipError, match="GPU only"):
        jpeg.decode_files([], "cpu")
