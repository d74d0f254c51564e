"""The YUV4MPEG2 reader without a GPU: the contract's arithmetic against float64, the header and FRAME-index parser through
_lib against tests/yuv_ref.py on the streams of tests/y4m_cases.py, every refusal by name, a stream cut at every byte, the
Reader's chunking, the writer, and Predictor.load_front_end's routing (cases 3b and 3c) with stubs."""
import ctypes as C
import io
import os
import sys
import threading
import types

import numpy as np
import pytest
import torch

import y4m_cases as yc
import yuv_ref
from poserisk_release_amd import _lib, dropin, frontend, y4m

dropin.install()
from core import base  # noqa: E402
from core.config import cfg  # noqa: E402

LAYOUTS = ("420jpeg", "420mpeg2", "422", "444")


# ---- the contract's arithmetic ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chroma", LAYOUTS)
@pytest.mark.parametrize("full", (False, True), ids=("limited", "full"))
@pytest.mark.parametrize("matrix", ("601", "709"))
def test_the_integer_contract_stays_within_one_level_of_float64(matrix, full, chroma):
    """Random 37x53 planes (W = 53, H = 37, three frames).  |integer - clip(float64)| < 1 everywhere, and the integer result is
    the rounded float64 result on at least 99.5 % of bytes: a condition (the contract alone gives 99.915 % or better here)."""
    Y, U, V = yc.planes(53, 37, chroma, F=3, seed=7)
    got = yuv_ref.convert(Y, U, V, chroma, matrix, full).astype(np.float64)
    exact = np.clip(yuv_ref.convert_f64(Y, U, V, chroma, matrix, full), 0, 255)
    worst = np.abs(got - exact).max()
    same = np.mean(got == np.clip(np.floor(exact + 0.5), 0, 255))
    print(f"{matrix} full={full} {chroma}: worst {worst:.4f} levels, {100 * same:.3f} % of bytes equal round(float64)")
    assert worst < 1.0
    assert same >= 0.995


@pytest.mark.parametrize("chroma", yuv_ref.CHROMAS)
def test_no_sum_leaves_int32_at_the_extreme_inputs(chroma):
    """Planes of 0 and 255 only, and the four constant corner cases: every sum of the matrix stays below 6.0e8 in magnitude
    (yuv_ref.convert asserts every partial sum against 2^31 as well)."""
    worst = 0
    for matrix in ("601", "709"):
        for full in (False, True):
            Y, U, V = yc.planes(16, 12, chroma, F=4, seed=1, kind="extreme")
            worst = max(worst, int(np.abs(yuv_ref.convert(Y, U, V, chroma, matrix, full, return_sums=True)).max()))
            for y in (0, 255):
                for u in (0, 255):
                    for v in (0, 255):
                        Yc = np.full((1, 4, 4), y, np.uint8)
                        Uc = None if chroma == "mono" else np.full((1,) + yuv_ref.chroma_size(4, 4, chroma)[::-1], u, np.uint8)
                        Vc = None if chroma == "mono" else np.full_like(Uc, v)
                        worst = max(worst, int(np.abs(yuv_ref.convert(Yc, Uc, Vc, chroma, matrix, full, return_sums=True)).max()))
    assert worst < 6.0e8, worst


def test_the_plan_is_the_contracts_and_the_abi_is_still_16():
    assert _lib.ABI_VERSION == 16 and _lib.load().pr_abi_version() == 16
    assert y4m.yuv_plan("601", False) == (76309, 104597, 132201, 25675, 53279, 16)
    for matrix in ("601", "709"):
        for full in (False, True):
            assert y4m.yuv_plan(matrix, full) == yuv_ref.plan(matrix, full)
    with pytest.raises(ValueError, match="matrix"):
        y4m.yuv_plan("2020", False)


def test_the_taps_of_every_axis_kind():
    c = np.array([[10, 20, 30]], np.uint8)                                  # one chroma row, cw = 3 -> W = 6
    cen = yuv_ref.chroma16(np.repeat(c, 1, 0), 6, 1, "420jpeg")[0] // 4      # the vertical axis of one row: 3 c + c = 4 c
    assert cen.tolist() == [4 * 10, 3 * 10 + 20, 3 * 20 + 10, 3 * 20 + 30, 3 * 30 + 20, 4 * 30]
    cos = yuv_ref.chroma16(c, 6, 1, "422")[0] // 4
    assert cos.tolist() == [4 * 10, 2 * 10 + 2 * 20, 4 * 20, 2 * 20 + 2 * 30, 4 * 30, 4 * 30]
    assert (yuv_ref.chroma16(c, 3, 1, "444")[0] == 16 * c[0].astype(np.int64)).all()


# ---- the parser -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c_field,chroma", yc.ACCEPTED_C, ids=[str(c) for c, _ in yc.ACCEPTED_C])
@pytest.mark.parametrize("colorrange,full", yc.RANGES, ids=[str(r) for r, _ in yc.RANGES])
def test_accepted_headers_and_the_frame_index_equal_the_reference(c_field, chroma, colorrange, full):
    Y, U, V = yc.planes(7, 5, chroma, F=5, seed=2)
    head = yc.header(7, 5, c_field, fps=(30000, 1001), interlace="p", aspect="1:1", colorrange=colorrange, extra=("XYSCSS=420JPEG", "Zq"))
    data, offsets = yc.stream(Y, U, V, head)
    assert yc.alignments(offsets) == {0, 1, 2, 3}
    info, ref = y4m.parse_header(data), yuv_ref.parse_header(data)
    assert info._asdict() == dict(ref, fps=30000 / 1001)
    assert (info.width, info.height, info.chroma, info.full_range, info.header_bytes) == (7, 5, chroma, full, len(head))
    assert info.frame_bytes == yuv_ref.frame_bytes(7, 5, chroma)
    got, used = y4m.index(data[len(head):], info)
    assert (got + len(head)).tolist() == offsets and used == len(data) - len(head)
    assert yuv_ref.index(data[len(head):], ref) == ((got).tolist(), used)
    two, used2 = y4m.index(data[len(head):], info, max_frames=2)
    assert two.tolist() == got[:2].tolist() and used2 == got[1] + info.frame_bytes


def test_frame_rate_defaults():
    assert y4m.parse_header(b"YUV4MPEG2 W4 H4\n").fps == 30.0
    assert y4m.parse_header(b"YUV4MPEG2 W4 H4 F0:0\n").fps == 30.0
    assert y4m.parse_header(b"YUV4MPEG2 W4 H4 F24:1\n").fps == 24.0
    assert y4m.parse_header(b"YUV4MPEG2 W4 H4 I? A0:0 XCOLORRANGE=WIDE\n").full_range is None


@pytest.mark.parametrize("case", yc.REFUSALS, ids=[f"{i}-{c[2]}" for i, c in enumerate(yc.REFUSALS)])
def test_every_refusal_by_name(case):
    head, word, code = case
    lib = _lib.load()
    info = _lib.Y4mInfo()
    C.memset(C.byref(info), 0x5A, C.sizeof(info))
    rc = lib.pr_y4m_parse_header(head, len(head), C.byref(info))
    assert rc == yc.CODES[code], (rc, code)
    assert bytes(info) == b"\x5a" * C.sizeof(info)                           # refused before anything is written
    assert word in y4m.refusal_name(rc) and word in lib.pr_last_error().decode()
    with pytest.raises(ValueError, match=word.replace(".", r"\.")):
        y4m.parse_header(head)
    with pytest.raises(ValueError):
        yuv_ref.parse_header(head)
    assert y4m.refusal_name(0) == "ok" and y4m.refusal_name(99) == "unknown refusal code"


def test_bytes_that_begin_no_frame_header_are_refused_with_the_frames_index():
    data, offsets, _ = yc.case(4, 4, "420jpeg", F=3, seed=0)
    info = y4m.parse_header(data)
    body = bytearray(data[info.header_bytes:])
    second = bytes(body).rfind(b"FRAME", 0, offsets[1] - info.header_bytes)
    for bad in (b"FRAMF", b"frame"):
        broken = bytes(body[:second]) + bad + bytes(body[second + 5:])
        with pytest.raises(ValueError, match="frame 1: no FRAME header"):
            y4m.index(broken, info)
        with pytest.raises(ValueError, match="frame 1"):
            yuv_ref.index(broken, yuv_ref.parse_header(data))
    with pytest.raises(ValueError, match="frame 0: no FRAME header"):
        y4m.index(b"FRAMEX\n" + bytes(24), info)
    with pytest.raises(ValueError, match="does not end within 256"):
        y4m.index(b"FRAME " + b"X" * 300 + b"\n" + bytes(24), info)


def test_a_buffer_cut_at_every_byte_of_a_two_frame_stream():
    Y, U, V = yc.planes(5, 3, "420mpeg2", F=2, seed=4)
    data, offsets = yc.stream(Y, U, V, yc.header(5, 3, "420mpeg2"), frame_fields=(b" Ip Xabc",))
    info, ref = y4m.parse_header(data), yuv_ref.parse_header(data)
    hb, fb = info.header_bytes, info.frame_bytes
    body = data[hb:]
    ends = [o - hb + fb for o in offsets]
    for cut in range(len(body) + 1):
        got, used = y4m.index(body[:cut], info)
        n = sum(cut >= e for e in ends)
        assert (len(got), used) == (n, ends[n - 1] if n else 0), cut
        assert got.tolist() == [o - hb for o in offsets[:n]]
        assert yuv_ref.index(body[:cut], ref) == (got.tolist(), used)
    for cut in range(hb):                                                     # and the header itself: refused until its '\n' is there
        with pytest.raises(ValueError):
            y4m.parse_header(data[:cut])


# ---- Reader and writer ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (1, 2, 3, 8))
def test_reader_chunks_from_bytes_a_file_and_a_pipe(n, tmp_path):
    data, offsets, _ = yc.case(9, 7, "420jpeg", F=5, seed=n, colorrange="FULL")
    path = tmp_path / "clip.y4m"
    path.write_bytes(data)
    assert y4m.is_y4m(path) and not y4m.is_y4m(tmp_path / "missing.y4m") and not y4m.is_y4m(__file__)
    r, w = os.pipe()

    def feed():
        with os.fdopen(w, "wb") as f:
            for lo in range(0, len(data), 50):                                # short writes: readinto returns short counts
                f.write(data[lo:lo + 50])
                f.flush()
    feeder = threading.Thread(target=feed)
    feeder.start()
    try:
        sources = {"bytes": io.BytesIO(data), "file": str(path), "pipe": os.fdopen(r, "rb")}
        for name, src in sources.items():
            with y4m.Reader(src) as reader:
                assert (reader.width, reader.height, reader.fps, reader.chroma, reader.full_range) == (9, 7, 25.0, "420jpeg", True)
                assert (reader.frames_bound is None) == (name == "pipe")
                payloads = []
                for chunk, offs in reader.chunks(n):
                    assert chunk.dtype == torch.uint8 and len(offs) <= n and bytes(chunk[:5].numpy()) == b"FRAME"
                    payloads += [bytes(chunk.numpy()[o:o + reader.info.frame_bytes]) for o in offs]
                assert payloads == [data[o:o + reader.info.frame_bytes] for o in offsets], name
                assert reader.frames_read == 5 and (reader.frames_bound is None or reader.frames_bound >= 5)
    finally:
        feeder.join()
        sources["pipe"].close()


def test_an_incomplete_last_frame_is_an_error_naming_its_index():
    data, offsets, _ = yc.case(9, 7, "422", F=3, seed=0)
    for cut in (offsets[2] + 10, offsets[2] - 3, len(data) - 1):
        with pytest.raises(ValueError, match="frame 2 is incomplete"):
            for _ in y4m.Reader(io.BytesIO(data[:cut])).chunks(2):
                pass
    with pytest.raises(ValueError, match="no YUV4MPEG2 signature"):
        y4m.Reader(io.BytesIO(b"RIFF1234AVI LIST"))


@pytest.mark.parametrize("chroma", yuv_ref.CHROMAS)
def test_write_then_read_gives_the_planes_back(chroma, tmp_path):
    Y, U, V = yc.planes(6, 5, chroma, F=3, seed=9)
    buf = io.BytesIO()
    y4m.write(buf, Y, U, V, fps=(30000, 1001), chroma=chroma, full_range=False)
    y4m.write(tmp_path / "w.y4m", Y, U, V, fps=29.97, chroma=chroma)
    info = yuv_ref.parse_header(buf.getvalue())
    assert (info["width"], info["height"], info["chroma"], info["full_range"], info["fps_num"], info["fps_den"]) == (6, 5, chroma, False, 30000, 1001)
    offsets, used = yuv_ref.index(buf.getvalue()[info["header_bytes"]:], info)
    assert len(offsets) == 3 and used + info["header_bytes"] == len(buf.getvalue())
    for k, o in enumerate(offsets):
        y, u, v = yuv_ref.planes_of(buf.getvalue(), info["header_bytes"] + o, 6, 5, chroma)
        assert np.array_equal(y, Y[k]) and (chroma == "mono" or (np.array_equal(u, U[k]) and np.array_equal(v, V[k])))
    other = y4m.parse_header((tmp_path / "w.y4m").read_bytes())
    assert other.full_range is None and abs(other.fps - 29.97) < 1e-3
    if chroma != "mono":
        with pytest.raises(ValueError, match="planes of 6 x 5 frames must be"):
            y4m.write(io.BytesIO(), Y, U[:, :1], V, chroma=chroma)


def test_decode_has_no_cpu_fallback():
    data, _, _ = yc.case(4, 4, "444", F=1)
    with pytest.raises(_lib.PoseRiskHipError, match="GPU only"):
        y4m.decode(data, "cpu")
    with pytest.raises(_lib.PoseRiskHipError, match="GPU only"):
        y4m.yuv_frames(torch.zeros(8, dtype=torch.uint8), torch.zeros(1, dtype=torch.int64), 2, 2, "mono", yuv_ref.plan("601", False))


# ---- load_front_end's routing, with stubs -----------------------------------------------------------------------------------------
@pytest.fixture()
def predictor(monkeypatch):
    """A Predictor that was never constructed (no model, no GPU): load_front_end only routes.  frontend.read_video is a stub that
    reads the stream to its end on the host and returns its frame count."""
    pred = base.Predictor.__new__(base.Predictor)
    pred.device, pred.video_decoder = torch.device("cpu"), ""
    calls = []

    def read_video(reader, device, **kw):
        assert isinstance(reader, y4m.Reader)
        frames = sum(len(offs) for _, offs in reader.chunks(2))
        calls.append((reader.path, frames, kw))
        return torch.zeros((frames, 2, 2, 3), dtype=torch.uint8), reader.fps
    monkeypatch.setattr(frontend, "read_video", read_video)
    monkeypatch.setitem(sys.modules, "cv2", None)
    monkeypatch.setitem(sys.modules, "multi_person_tracker", None)
    return pred, calls


def test_a_y4m_file_takes_case_3b(predictor, tmp_path, monkeypatch):
    pred, calls = predictor
    assert cfg.DATASET.yuv_matrix == "601" and cfg.DATASET.video_decoder == ""
    data, _, _ = yc.case(8, 6, "420jpeg", F=3, fps=(24, 1))
    clip = tmp_path / "clip.y4m"
    clip.write_bytes(data)
    track = {1: {"bbox": np.zeros((1, 4), np.float32), "frames": np.array([0])}}
    frames, bgr, fps, tracking = pred.load_front_end(str(clip), str(tmp_path / "out"), tracking_results=track)
    assert frames.shape[0] == 3 and bgr is False and fps == 24.0 and tracking is track
    assert calls == [(str(clip), 3, dict(max_w=800, max_h=450, matrix="601"))]
    monkeypatch.setitem(cfg.DATASET, "yuv_matrix", "709")
    import pickle
    with open(tmp_path / "clip.tracking.pkl", "wb") as f:
        pickle.dump({5: {"bbox": np.ones((1, 4), np.float32), "frames": np.array([2])}}, f)
    _, _, _, tracking = pred.load_front_end(str(clip), str(tmp_path / "out"))
    assert list(tracking) == [5] and calls[-1][2]["matrix"] == "709"
    os.remove(tmp_path / "clip.tracking.pkl")
    with pytest.raises(RuntimeError, match=r"clip\.tracking\.pkl.*frontend prepare .*clip\.y4m"):     # the AVI case's own named error
        pred.load_front_end(str(clip), str(tmp_path / "out"))


def test_another_file_with_the_knob_off_reaches_the_old_error_unchanged(predictor, tmp_path):
    pred, calls = predictor
    other = tmp_path / "clip.mp4"
    other.write_bytes(b"\0\0\0\x18ftypmp42" + bytes(64))
    with pytest.raises(RuntimeError, match=r"clip\.mp4' is neither a directory with frames\.npy \+ tracking\.pkl nor one with JPEG frames "
                                         r"\(\*\.jpg, decoded on the GPU\) or PNG frames \(\*\.png, decoded on the GPU\) \+ tracking\.pkl, and the "
                                         r"reference's front end \(cv2 video decoding, multi_person_tracker\) is not importable here .* "
                                         r"then call Predictor\.score_frames\(frames, tracking_results, info\)$"):
        pred.load_front_end(str(other), str(tmp_path / "out"))
    assert calls == []


def test_the_decoder_command_runs_once_as_a_child_and_its_output_is_read_as_y4m(predictor, tmp_path):
    pred, calls = predictor
    data, _, _ = yc.case(8, 6, "420mpeg2", F=5, fps=(12, 1))
    (tmp_path / "stream.bin").write_bytes(data)
    script = tmp_path / "decoder.py"
    script.write_text("import sys\n"
                      "open(sys.argv[2], 'a').write(sys.argv[1] + '\\n')\n"
                      "sys.stdout.buffer.write(open(sys.argv[3], 'rb').read())\n")
    other = tmp_path / "my clip.mp4"                                          # a space: no shell splits it
    other.write_bytes(b"\0\0\0\x18ftypmp42" + bytes(64))
    import shlex
    pred.video_decoder = " ".join(shlex.quote(str(a)) for a in (sys.executable, script, "{input}", tmp_path / "runs.txt", tmp_path / "stream.bin"))
    track = {1: {"bbox": np.zeros((1, 4), np.float32), "frames": np.array([0])}}
    frames, bgr, fps, tracking = pred.load_front_end(str(other), str(tmp_path / "out"), tracking_results=track)
    assert frames.shape[0] == 5 and bgr is False and fps == 12.0 and tracking is track
    assert (tmp_path / "runs.txt").read_text() == str(other) + "\n"           # once, with the input's own path
    assert len(calls) == 1 and calls[0][1] == 5
    # a Y4M file and a directory never reach the command
    clip = tmp_path / "clip.y4m"
    clip.write_bytes(data)
    pred.load_front_end(str(clip), str(tmp_path / "out"), tracking_results=track)
    assert (tmp_path / "runs.txt").read_text() == str(other) + "\n" and calls[-1][0] == str(clip)
    pred.video_decoder = "cat"
    with pytest.raises(ValueError, match="must be a command line containing {input}"):
        pred.load_front_end(str(other), str(tmp_path / "out"), tracking_results=track)


def test_a_failing_decoder_raises_with_its_status_and_the_tail_of_its_stderr(predictor, tmp_path):
    pred, calls = predictor
    data, _, _ = yc.case(8, 6, "420jpeg", F=3)
    (tmp_path / "stream.bin").write_bytes(data)
    other = tmp_path / "clip.mkv"
    other.write_bytes(bytes(64))
    track = {1: {"bbox": np.zeros((1, 4), np.float32), "frames": np.array([0])}}
    script = tmp_path / "decoder.py"
    import shlex
    command = lambda *extra: " ".join(shlex.quote(str(a)) for a in (sys.executable, script, "{input}", *extra))
    # no header at all
    script.write_text("import sys\nsys.stderr.write('x' * 5000 + ' moov atom not found\\n')\nsys.exit(3)\n")
    pred.video_decoder = command()
    with pytest.raises(RuntimeError, match=r"clip\.mkv.*decoder\.py.*exit status 3.*wrote no YUV4MPEG2 stream header.*moov atom not found") as e:
        pred.load_front_end(str(other), str(tmp_path / "out"), tracking_results=track)
    assert len(str(e.value)) < 4000                                           # the tail, not all of it
    # a whole stream, then a non-zero status
    script.write_text("import sys\nsys.stdout.buffer.write(open(sys.argv[2], 'rb').read())\nsys.stdout.flush()\n"
                      "sys.stderr.write('late failure\\n')\nsys.exit(7)\n")
    pred.video_decoder = command(tmp_path / "stream.bin")
    with pytest.raises(RuntimeError, match=r"exit status 7.*late failure"):
        pred.load_front_end(str(other), str(tmp_path / "out"), tracking_results=track)
    # a stream that breaks off inside frame 2, status 0: still an error, naming the frame
    script.write_text("import sys\nsys.stdout.buffer.write(open(sys.argv[2], 'rb').read()[:-5])\n")
    with pytest.raises(RuntimeError, match=r"exit status 0.*frame 2 is incomplete"):
        pred.load_front_end(str(other), str(tmp_path / "out"), tracking_results=track)
    # a program that does not exist
    pred.video_decoder = str(tmp_path / "no-such-decoder") + " {input}"
    with pytest.raises(RuntimeError, match="could not be started"):
        pred.load_front_end(str(other), str(tmp_path / "out"), tracking_results=track)
    assert calls == [] or all(c[1] == 3 for c in calls)


def test_a_dash_reads_standard_input(monkeypatch):
    data, offsets, _ = yc.case(6, 4, "444", F=2, seed=1)
    monkeypatch.setattr(sys, "stdin", types.SimpleNamespace(buffer=io.BytesIO(data)))
    reader = frontend._y4m_source("-")
    assert isinstance(reader, y4m.Reader) and reader.path == "<stdin>" and (reader.width, reader.height, reader.chroma) == (6, 4, "444")
    assert sum(len(offs) for _, offs in reader.chunks(4)) == 2
    assert frontend._y4m_source(__file__) is None and frontend._y4m_source("no-such-file.y4m") is None
