"""The YUV4MPEG2 writer on the GPU: pr_yuv_encode inside guard bands against tests/yuv_enc_ref.py with the output at every byte
alignment, extreme colours, the round trip through y4m.decode, a second call that allocates nothing, a captured graph,
y4m.Writer to a file, an object and a child process, and the Predictor's 'y4m' codec and video_encoder knob."""
import ctypes as C
import io
import pickle
import sys
import types

import numpy as np
import pytest
import torch

import guard_band as gb
import yuv_enc_ref as er
from poserisk_release_amd import _lib, synth, video, y4m

pytestmark = pytest.mark.gpu
F = 3                                                                      # frames a call: they begin at different alignments
SIZES = ((3, 3), (7, 5), (17, 13), (64, 2))                                # (W, H)
COPY = "import sys, shutil; shutil.copyfileobj(sys.stdin.buffer, open(sys.argv[1], 'wb'))"
# (matrix, full_range, bgr, (pad_h, pad_w)): the first at every alignment of dst, the others at one alignment each
EVERYWHERE = ("601", False, False, (1, 1))
ROTATING = (("601", True, True, (0, 0)), ("709", False, True, (1, 0)), ("709", True, False, (0, 1)), ("601", False, True, (0, 0)))


def _first_difference(got, want):
    got, want = np.frombuffer(got, np.uint8), np.frombuffer(want, np.uint8)
    if got.size != want.size:
        return f"{got.size} bytes for {want.size}"
    bad = np.nonzero(got != want)[0]
    return f"{bad.size} bytes differ, first at byte {bad[0]}: {got[bad[0]]} for {want[bad[0]]}"


def _guarded(device, frames, chroma, matrix="601", full=False, bgr=False, out=None, shift=0):
    """pr_yuv_encode with src and dst each in the middle of an arena, dst's first byte `shift` bytes behind an aligned address:
    the bytes of the arena's view in front of and behind the output must keep their canary too.  -> the call's bytes."""
    n, H, W, _ = frames.shape
    oh, ow = out or (H, W)
    total = n * (6 + er.frame_bytes(ow, oh, chroma))
    lib = _lib.load()

    def call(i, o):
        assert o["dst"].data_ptr() % 4 == 0
        a = _lib.YuvEncArgs()
        a.src, a.dst = i["src"].data_ptr(), o["dst"].data_ptr() + shift
        a.plan = _lib.YuvEncCoeffs(*er.plan(matrix, full))
        a.F, a.H, a.W, a.out_H, a.out_W, a.chroma, a.bgr = n, H, W, oh, ow, y4m.CHROMAS.index(chroma), int(bgr)
        _lib.check(lib.pr_yuv_encode(C.byref(a), torch.cuda.current_stream(device).cuda_stream), "pr_yuv_encode")
    outs = gb.run_guarded(call, {"src": torch.from_numpy(np.ascontiguousarray(frames))}, {"dst": ((total + 3,), torch.uint8)},
                          device=device, may_hold_canary=("dst",))
    got = outs["dst"].cpu().numpy()
    assert (got[:shift] == gb.CANARY_U8).all() and (got[shift + total:] == gb.CANARY_U8).all(), f"bytes around dst written, alignment {shift}"
    return got[shift:shift + total].tobytes()


# ---- the kernel ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chroma", er.CHROMAS)
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_encode_equals_the_reference_inside_guard_bands_at_every_alignment(gpu_device, chroma, size):
    W, H = size
    frames = np.random.default_rng(W * 100 + H).integers(0, 256, (F, H, W, 3), dtype=np.uint8)
    for shift in range(4):
        for matrix, full, bgr, (ph, pw) in (EVERYWHERE, ROTATING[shift]):
            out = (H + ph, W + pw)
            got = _guarded(gpu_device, frames, chroma, matrix, full, bgr, out, shift)
            want = er.encode(frames, chroma, matrix, full, bgr, out)
            assert got == want, (f"{matrix} full={full} bgr={bgr} padded to {out[1]}x{out[0]}, dst at alignment {shift}: "
                                 + _first_difference(got, want))


@pytest.mark.parametrize("chroma", er.CHROMAS)
def test_extreme_colours(gpu_device, chroma):
    """Pure primaries, black and white as flat frames, and 0 / 255 noise, where chroma reaches the ends of its range."""
    rng = np.random.default_rng(2)
    flat = np.array([[255, 0, 0], [0, 255, 0], [0, 0, 255], [0, 0, 0], [255, 255, 255]], np.uint8)
    frames = np.concatenate([np.broadcast_to(flat[:, None, None, :], (5, 5, 7, 3)), (255 * rng.integers(0, 2, (2, 5, 7, 3))).astype(np.uint8)])
    for matrix in ("601", "709"):
        for full in (False, True):
            got = _guarded(gpu_device, frames, chroma, matrix, full, out=(6, 8), shift=1)
            want = er.encode(frames, chroma, matrix, full, out_size=(6, 8))
            assert got == want, (matrix, full, _first_difference(got, want))
    Y, U, V = er.planes(frames[3:5], chroma, "601", False)
    assert (Y[0] == 16).all() and (Y[1] == 235).all() and (U is None or ((U == 128).all() and (V == 128).all()))


def _round_trip(device, frames, chroma, matrix, full):
    """frames u8[F,H,W,3] (numpy) -> worst |decode(header + encode_frames) - frames| per channel, over the source's area."""
    n, H, W, _ = frames.shape
    body = y4m.encode_frames(torch.from_numpy(frames).to(device), chroma, matrix, full, pad_even=True)
    ow, oh, size = y4m.encoded_size(W, H, chroma, pad_even=True)
    assert tuple(body.shape) == (n, size)
    stream = y4m.stream_header(ow, oh, 30.0, chroma, full) + body.cpu().numpy().tobytes()
    back = y4m.decode(stream, device, matrix=matrix).cpu().numpy()
    assert back.shape == (n, oh, ow, 3)
    return np.abs(back[:, :H, :W].astype(np.int64) - frames).reshape(-1, 3).max(axis=0).tolist()


@pytest.mark.parametrize("chroma", ("420jpeg", "420mpeg2", "422", "444"))
def test_flat_colour_frames_come_back_within_the_contracts_bound(gpu_device, chroma):
    """64 flat frames of 7x5 (padded to 8x6) in random colours plus the cube's corners: subsampling is the identity there, so
    the 444 bound holds: 1 level in full range; 1 for R and G, 2 for B in limited range.  (mono keeps no colour to return.)"""
    rng = np.random.default_rng(5)
    corners = np.array([[r, g, b] for r in (0, 255) for g in (0, 255) for b in (0, 255)], np.uint8)
    colours = np.concatenate([corners, rng.integers(0, 256, (56, 3), dtype=np.uint8)])
    frames = np.ascontiguousarray(np.broadcast_to(colours[:, None, None, :], (64, 5, 7, 3)))
    for matrix in ("601", "709"):
        for full in (False, True):
            worst = _round_trip(gpu_device, frames, chroma, matrix, full)
            assert all(w <= b for w, b in zip(worst, (1, 1, 1) if full else (1, 1, 2))), (matrix, full, worst)


def test_random_444_frames_come_back_within_the_contracts_bound(gpu_device):
    frames = np.random.default_rng(6).integers(0, 256, (F, 13, 17, 3), dtype=np.uint8)
    for matrix in ("601", "709"):
        for full in (False, True):
            worst = _round_trip(gpu_device, frames, "444", matrix, full)
            assert all(w <= b for w, b in zip(worst, (1, 1, 1) if full else (1, 1, 2))), (matrix, full, worst)


def test_a_second_call_with_out_allocates_nothing_and_a_graph_replays_the_same_bytes(gpu_device):
    frames = np.random.default_rng(7).integers(0, 256, (F, 13, 17, 3), dtype=np.uint8)
    want = er.encode(frames, "420mpeg2", out_size=(14, 18))
    dev = torch.from_numpy(frames).to(gpu_device)
    first = y4m.encode_frames(dev, pad_even=True)
    outs = [torch.zeros_like(first) for _ in range(2)]
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated(gpu_device)
    assert y4m.encode_frames(dev, pad_even=True, out=outs[0]) is outs[0]
    assert torch.cuda.memory_allocated(gpu_device) == before
    torch.cuda.synchronize()
    assert torch.equal(outs[0], first) and first.cpu().numpy().tobytes() == want
    side = torch.cuda.Stream(gpu_device)
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            y4m.encode_frames(dev, pad_even=True, out=outs[1])
    for _ in range(2):
        outs[1].zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(outs[1], first)


def test_argument_errors_are_named(gpu_device):
    dev = torch.zeros((1, 4, 4, 3), dtype=torch.uint8, device=gpu_device)
    with pytest.raises(ValueError, match="out must be"):
        y4m.encode_frames(dev, out=torch.empty((1, 5), dtype=torch.uint8, device=gpu_device))
    with pytest.raises(ValueError, match="is not one of"):
        y4m.encode_frames(dev, chroma="411")
    with pytest.raises(ValueError, match="contiguous uint8"):
        y4m.encode_frames(dev.float())
    with pytest.raises(_lib.PoseRiskHipError, match="every side must lie in 1..4096"):
        y4m.encode_frames(torch.zeros((1, 1, 4097, 3), dtype=torch.uint8, device=gpu_device))
    assert y4m.encode_frames(dev[:0]).shape == (0, 6 + 16 + 8)


# ---- the Writer ---------------------------------------------------------------------------------------------------------------
def test_writer_to_a_file_an_object_and_a_child_gives_identical_bytes(gpu_device, tmp_path):
    """Seven frames of 17x13 in batches of 3, 3 and 1: both pinned buffers are used twice."""
    frames = np.random.default_rng(8).integers(0, 256, (7, 13, 17, 3), dtype=np.uint8)
    dev = torch.from_numpy(frames).to(gpu_device)
    want = y4m.stream_header(18, 14, (24, 1), "420mpeg2", False) + er.encode(frames, "420mpeg2", "709", False, True, (14, 18))
    how = dict(width=17, height=13, fps=(24, 1), matrix="709", bgr=True, pad_even=True)
    mem = io.BytesIO()
    sinks = [(y4m.Writer(str(tmp_path / "a.y4m"), **how), lambda: (tmp_path / "a.y4m").read_bytes()),
             (y4m.Writer(mem, **how), mem.getvalue),
             (y4m.Writer(command=[sys.executable, "-c", COPY, str(tmp_path / "b.y4m")], **how), lambda: (tmp_path / "b.y4m").read_bytes())]
    for w, read in sinks:
        for lo in (0, 3, 6):
            w.put(dev[lo:lo + 3])
        assert w.frames_written == 6                          # the last batch waits for close
        w.close()
        got = read()
        assert w.frames_written == 7 and got == want, _first_difference(got, want)
    back = y4m.decode(want, gpu_device, matrix="709", bgr=True)
    assert tuple(back.shape) == (7, 14, 18, 3)
    with pytest.raises(ValueError, match=r"frames must be \[F,13,17,3\]"):
        y4m.Writer(io.BytesIO(), **how).put(dev[:, :12])


# ---- Predictor.__call__ with the 'y4m' codec and the video_encoder knob ---------------------------------------------------------
def _predictor(gpu_device, **knobs):
    from poserisk_release_amd import dropin
    dropin.install()
    from core import base
    from models import hmr
    from smpl import SMPL
    model = hmr()
    model.load_state_dict(synth.hmr_state_dict(seed=1), strict=False)
    sm = synth.smpl_model(V=6890, seed=2)
    sm["f"] = synth.genus0_mesh(6890)[1]
    smpl = SMPL(models={"neutral": sm}, device=gpu_device)
    args = types.SimpleNamespace(gpu="0", type="REBA", debug=False, debug_joints="", debug_frame=-1, **knobs)
    return base.Predictor(args, spin_model=model, smpl_model=smpl, batch_size=4)


def _clip(tmp_path):
    """Six frames of 320 x 180 (the smallest the Predictor's tests use), a track over frames 0-2, 4 and 5."""
    frames = np.random.default_rng(9).integers(0, 256, (6, 180, 320, 3), dtype=np.uint8)
    fr = [0, 1, 2, 4, 5]
    tr = {3: {'bbox': np.stack([np.array([150 + 4 * i, 90 - i, 70, 130], np.float32) for i in range(len(fr))]), 'frames': np.array(fr)}}
    src = tmp_path / "clip"
    src.mkdir()
    np.save(src / "frames.npy", frames)
    with open(src / "tracking.pkl", "wb") as f:
        pickle.dump(tr, f)
    return frames, str(src)


def test_predictor_writes_y4m_and_feeds_an_encoder_the_same_stream(gpu_device, tmp_path, monkeypatch):
    monkeypatch.setitem(sys.modules, "cv2", None)              # with or without cv2
    frames, src = _clip(tmp_path)
    pred = _predictor(gpu_device, gpu_video=True, video_codec="y4m")
    assert pred.gpu_video_codec == "y4m" and pred.video_encoder == "" and pred.video_chroma == "420mpeg2"
    out = pred(src, "", str(tmp_path / "out"))
    names = sorted(p.name for p in (tmp_path / "out").iterdir())
    assert "REBA_video.y4m" in names and "REBA_video" not in names and "REBA_video.mp4" not in names
    data = (tmp_path / "out" / "REBA_video.y4m").read_bytes()
    canvas_h, resize_w, panel_w = video.canvas_size(180, 320)
    W, H = resize_w + panel_w, canvas_h
    info = y4m.parse_header(data)
    assert (info.width, info.height) == (W + (W & 1), H + (H & 1)) and info.width % 2 == 0 and info.height % 2 == 0
    assert (info.chroma, info.full_range) == ("420mpeg2", False) and abs(info.fps - float(out["fps"])) < 1e-3
    assert len(data) == info.header_bytes + 6 * (6 + info.frame_bytes)                       # one frame per video frame
    decoded = y4m.decode(data, gpu_device)
    assert tuple(decoded.shape) == (6, info.height, info.width, 3)
    # the stream is the device encoder's: the canvases composed again, through the numpy reference
    _, scores, logs, _ = out["reba"]
    draw = video.draw_list("REBA", 6, out['bboxes'], (0, out['frames'], 6), scores, pred.reba.eval_items, logs, canvas_h)
    canvases = torch.cat(list(video.annotated_frames(torch.from_numpy(frames).to(gpu_device), draw, 4))).cpu().numpy()
    want = er.encode(canvases, "420mpeg2", "601", False, False, (info.height, info.width))
    assert data[info.header_bytes:] == want, _first_difference(data[info.header_bytes:], want)

    # the same stream through an encoder child: one that copies its standard input to {output}
    piped = _predictor(gpu_device, gpu_video=True, video_encoder=f"{sys.executable} -c \"{COPY}\" {{output}}", video_encoder_ext=".y4m")
    assert piped.gpu_video_codec == "y4m"                      # implied
    piped(src, "", str(tmp_path / "piped"))
    assert (tmp_path / "piped" / "REBA_video.y4m").read_bytes() == data
    default_ext = _predictor(gpu_device, gpu_video=True, video_encoder=f"{sys.executable} -c \"{COPY}\" {{output}}")
    assert default_ext.video_encoder_ext == ".mp4"

    failing = _predictor(gpu_device, gpu_video=True,
                         video_encoder=f"{sys.executable} -c \"import sys; sys.stdin.buffer.read(); sys.stderr.write('unknown encoder'); sys.exit(7)\" {{output}}")
    with pytest.raises(RuntimeError, match=r"(?s)failed with exit status 7.*unknown encoder"):
        failing(src, "", str(tmp_path / "failing"))
    with pytest.raises(ValueError, match=r"must be a command line containing \{output\}"):
        _predictor(gpu_device, gpu_video=True, video_encoder="ffmpeg -i - out.mp4")
    with pytest.raises(ValueError, match="goes with gpu_video_codec 'y4m'"):
        _predictor(gpu_device, gpu_video=True, video_codec="mjpeg", video_encoder="enc {output}")
    with pytest.raises(ValueError, match="h264"):
        _predictor(gpu_device, gpu_video=True, video_codec="h264")


def test_predictor_writes_the_mesh_as_y4m_too(gpu_device, tmp_path, monkeypatch):
    monkeypatch.setitem(sys.modules, "cv2", None)
    from poserisk_release_amd import dropin
    dropin.install()
    from core.config import cfg
    frames, src = _clip(tmp_path)
    monkeypatch.setitem(cfg.DATASET, "video_chroma", "444")
    pred = _predictor(gpu_device, gpu_video=True, render_mesh=True, video_codec="y4m")
    out = pred(src, "", str(tmp_path / "out"))
    mesh = (tmp_path / "out" / "REBA_mesh.y4m").read_bytes()
    info = y4m.parse_header(mesh)
    assert (info.width, info.height, info.chroma) == (320, 180, "444")                       # 444: nothing to pad
    assert len(mesh) == info.header_bytes + len(out["frames"]) * (6 + info.frame_bytes)
    assert y4m.parse_header((tmp_path / "out" / "REBA_video.y4m").read_bytes()).chroma == "444"
