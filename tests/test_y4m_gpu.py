"""The YUV4MPEG2 reader on the GPU: pr_yuv_frames inside guard bands against tests/yuv_ref.py, the fused downscale against the
two-step path, y4m.decode from bytes, a file and a pipe, frontend.read_video, the Predictor on a `.y4m` with a tracking sidecar,
and a second call that allocates nothing."""
import ctypes as C
import json
import os
import pickle
import sys
import threading
import types

import numpy as np
import pytest
import torch

import guard_band as gb
import resize_ref as rr
import y4m_cases as yc
import yuv_ref
from poserisk_release_amd import _lib, dropin, frontend, synth, y4m

dropin.install()
from core import base  # noqa: E402
from core.config import cfg  # noqa: E402
from models import hmr  # noqa: E402
from smpl import SMPL  # noqa: E402

pytestmark = pytest.mark.gpu
F = 3                                                                      # frames a call
FUSED_PAIRS = (((37, 53), (37, 53)), ((20, 32), (10, 16)), ((37, 53), (17, 23)))     # (H, W) -> (h, w): COPY, HALF, LINEAR
FUSED_IDS = ("copy", "half", "linear")


def _first_difference(got, want):
    bad = np.argwhere(got != want)
    return f"{len(bad)} bytes differ, first (frame, row, col, channel) {bad[0].tolist()}: {got[tuple(bad[0])]} for {want[tuple(bad[0])]}"


def _stream(W, H, chroma, seed, frames=F, kind="noise"):
    """-> (the stream as a uint8 tensor, payload offsets int64 tensor, planes)"""
    data, offsets, planes = yc.case(W, H, chroma, F=frames, seed=seed, kind=kind)
    assert len(yc.alignments(offsets)) == min(frames, 4)
    return torch.from_numpy(np.frombuffer(data, np.uint8).copy()), torch.tensor(offsets, dtype=torch.int64), planes


def _guarded(device, data, offsets, H, W, chroma, plan, bgr=False, size=None, may_hold_canary=True):
    """pr_yuv_frames with the stream, the offsets, the tables and the output each in the middle of an arena.  The offsets travel
    as the int32 words they are stored in (guard_band knows int32 and uint8)."""
    h, w = size or (H, W)
    ins = {"data": data, "offsets": offsets.view(torch.int32)}
    mode = 0
    if size is not None:
        xofs, xcoef, yofs, ycoef, mode = frontend.resize_plan(H, W, h, w)
        ins.update(xofs=torch.from_numpy(xofs), xcoef=torch.from_numpy(xcoef.view(np.int32).copy()),
                   yofs=torch.from_numpy(yofs), ycoef=torch.from_numpy(ycoef.view(np.int32).copy()))
    lib = _lib.load()

    def call(i, o):
        a = _lib.YuvArgs()
        a.data, a.data_bytes, a.offsets, a.dst = i["data"].data_ptr(), data.numel(), i["offsets"].data_ptr(), o["dst"].data_ptr()
        a.plan = _lib.YuvCoeffs(*plan)
        a.F, a.H, a.W, a.chroma, a.bgr = offsets.numel(), H, W, y4m.CHROMAS.index(chroma), int(bgr)
        if size is not None:
            a.xofs, a.xcoef, a.yofs, a.ycoef = (i[k].data_ptr() for k in ("xofs", "xcoef", "yofs", "ycoef"))
            a.h, a.w, a.mode = h, w, mode
        _lib.check(lib.pr_yuv_frames(C.byref(a), torch.cuda.current_stream(device).cuda_stream), "pr_yuv_frames")
    outs = gb.run_guarded(call, ins, {"dst": ((offsets.numel(), h, w, 3), torch.uint8)}, device=device,
                          may_hold_canary=("dst",) if may_hold_canary else ())
    return outs["dst"].cpu().numpy()


# ---- the kernel ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chroma", yuv_ref.CHROMAS)
@pytest.mark.parametrize("size", yc.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_yuv_frames_equals_the_reference_inside_guard_bands(gpu_device, chroma, size):
    """Three frames a call whose payloads start at three byte alignments of the chunk (a fourth frame's at the fourth in the
    37x53 case), both matrices and ranges, bgr."""
    W, H = size
    frames = 4 if size == (37, 53) else F
    data, offsets, (Y, U, V) = _stream(W, H, chroma, seed=W * 100 + H, frames=frames)
    for matrix, full, bgr in (("601", False, False), ("601", True, True), ("709", False, True), ("709", True, False)):
        got = _guarded(gpu_device, data, offsets, H, W, chroma, yuv_ref.plan(matrix, full), bgr)
        want = yuv_ref.convert(Y, U, V, chroma, matrix, full, bgr)
        assert np.array_equal(got, want), (matrix, full, bgr, _first_difference(got, want))


@pytest.mark.parametrize("chroma", yuv_ref.CHROMAS)
def test_every_output_byte_is_written_and_extremes_clamp(gpu_device, chroma):
    """Constant planes whose RGB holds no canary byte: nothing may stay unwritten; then 0 / 255 planes, where R, G and B clamp."""
    W, H = 53, 37
    cw, ch = yuv_ref.chroma_size(W, H, chroma)
    Y = np.full((F, H, W), 120, np.uint8)
    U = V = None if chroma == "mono" else np.full((F, ch, cw), 128, np.uint8)
    raw, offs = yc.stream(Y, U, V, yc.header(W, H, chroma))
    want = yuv_ref.convert(Y, U, V, chroma)
    assert not (want == gb.CANARY_U8).any()
    data, offsets = torch.from_numpy(np.frombuffer(raw, np.uint8).copy()), torch.tensor(offs, dtype=torch.int64)
    got = _guarded(gpu_device, data, offsets, H, W, chroma, yuv_ref.plan("601", False), may_hold_canary=False)
    assert np.array_equal(got, want)
    got = _guarded(gpu_device, data, offsets, H, W, chroma, yuv_ref.plan("601", False), size=(17, 23), may_hold_canary=False)
    assert np.array_equal(got, rr.resize(want, 17, 23))
    data, offsets, (Y, U, V) = _stream(W, H, chroma, seed=5, kind="extreme")
    got = _guarded(gpu_device, data, offsets, H, W, chroma, yuv_ref.plan("709", False))
    assert np.array_equal(got, yuv_ref.convert(Y, U, V, chroma, "709", False))


@pytest.mark.parametrize("chroma", yuv_ref.CHROMAS)
@pytest.mark.parametrize("pair", FUSED_PAIRS, ids=FUSED_IDS)
def test_fused_equals_unfused_then_resize_frames_bit_for_bit(gpu_device, chroma, pair):
    """COPY, HALF (32x20 -> 16x10), LINEAR (53x37 -> 23x17: 1173 bytes a frame, later frames start unaligned); in guard bands,
    against the reference, and through y4m.yuv_frames against frontend.resize_frames of its own source-size output; then with
    the output's first byte at alignments 1, 2 and 3."""
    (H, W), (h, w) = pair
    data, offsets, (Y, U, V) = _stream(W, H, chroma, seed=H + w)
    plan = yuv_ref.plan("601", False)
    want = rr.resize(yuv_ref.convert(Y, U, V, chroma), h, w)
    got = _guarded(gpu_device, data, offsets, H, W, chroma, plan, size=(h, w))
    assert np.array_equal(got, want), _first_difference(got, want)
    d, o = data.to(gpu_device), offsets.to(gpu_device)
    rgb = y4m.yuv_frames(d, o, H, W, chroma, plan)
    two_step = frontend.resize_frames(rgb, h, w)
    fused = y4m.yuv_frames(d, o, H, W, chroma, plan, size=(h, w))
    assert torch.equal(fused, two_step) and np.array_equal(fused.cpu().numpy(), want)
    n = F * h * w * 3
    for shift in (1, 2, 3):
        big = torch.full((n + 8,), 0x5A, dtype=torch.uint8, device=gpu_device)
        assert big.data_ptr() % 4 == 0
        out = big[shift:shift + n].view(F, h, w, 3)
        assert y4m.yuv_frames(d, o, H, W, chroma, plan, size=(h, w), out=out) is out
        assert torch.equal(out, two_step), shift
        assert bool((big[:shift] == 0x5A).all()) and bool((big[shift + n:] == 0x5A).all()), shift


def test_a_payload_outside_the_chunk_is_zeros_and_argument_errors_are_named(gpu_device):
    data, offsets, (Y, U, V) = _stream(7, 5, "420jpeg", seed=1)
    plan = yuv_ref.plan("601", False)
    fb = yuv_ref.frame_bytes(7, 5, "420jpeg")
    bad = offsets.clone()
    bad[1] = data.numel() - fb + 1
    got = _guarded(gpu_device, data, bad, 5, 7, "420jpeg", plan)
    want = yuv_ref.convert(Y, U, V, "420jpeg")
    want[1] = 0
    assert np.array_equal(got, want)
    d, o = data.to(gpu_device), offsets.to(gpu_device)
    with pytest.raises(_lib.PoseRiskHipError, match="every side must lie in 1..4096"):
        y4m.yuv_frames(d, o, 5, 5000, "420jpeg", plan)
    with pytest.raises(ValueError, match="out must be"):
        y4m.yuv_frames(d, o, 5, 7, "420jpeg", plan, out=torch.empty((F, 5, 8, 3), dtype=torch.uint8, device=gpu_device))
    with pytest.raises(ValueError, match="offsets must be"):
        y4m.yuv_frames(d, o.to(torch.int32), 5, 7, "420jpeg", plan)
    assert y4m.yuv_frames(d, o[:0], 5, 7, "420jpeg", plan).shape == (0, 5, 7, 3)


def test_a_second_call_with_out_and_tables_made_allocates_nothing(gpu_device):
    (H, W), (h, w) = FUSED_PAIRS[2]
    data, offsets, _ = _stream(W, H, "420mpeg2", seed=3)
    d, o = data.to(gpu_device), offsets.to(gpu_device)
    plan = yuv_ref.plan("601", False)
    out = torch.empty((F, h, w, 3), dtype=torch.uint8, device=gpu_device)
    first = y4m.yuv_frames(d, o, H, W, "420mpeg2", plan, size=(h, w)).clone()
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated(gpu_device)
    y4m.yuv_frames(d, o, H, W, "420mpeg2", plan, size=(h, w), out=out)
    assert torch.cuda.memory_allocated(gpu_device) == before
    torch.cuda.synchronize()
    assert torch.equal(out, first)


# ---- decode and read_video ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fused", (True, False), ids=("fused", "two-step"))
def test_decode_from_bytes_a_file_and_a_pipe_gives_equal_tensors(gpu_device, fused, tmp_path):
    """Five frames of 54x30 420mpeg2 with XCOLORRANGE=FULL; chunks of 2, so a chunk boundary falls inside a frame's bytes."""
    data, _, (Y, U, V) = yc.case(54, 30, "420mpeg2", F=5, seed=8, colorrange="FULL")
    path = tmp_path / "clip.y4m"
    path.write_bytes(data)
    want = yuv_ref.convert(Y, U, V, "420mpeg2", "601", True)
    whole = y4m.decode(data, gpu_device, fused=fused)
    assert whole.shape == (5, 30, 54, 3) and np.array_equal(whole.cpu().numpy(), want), _first_difference(whole.cpu().numpy(), want)
    assert torch.equal(y4m.decode(data, gpu_device, chunk=2, fused=fused), whole)
    assert torch.equal(y4m.decode(str(path), gpu_device, chunk=2, fused=fused), whole)
    r, w = os.pipe()

    def feed():
        with os.fdopen(w, "wb") as f:
            for lo in range(0, len(data), 1000):
                f.write(data[lo:lo + 1000])
                f.flush()
    feeder = threading.Thread(target=feed)
    feeder.start()
    try:
        with os.fdopen(r, "rb") as pipe:
            piped = y4m.decode(pipe, gpu_device, chunk=2, fused=fused)
    finally:
        feeder.join()
    assert torch.equal(piped, whole)
    small = y4m.decode(data, gpu_device, size=(15, 27), chunk=2, fused=fused, bgr=True, full_range=False, matrix="709")
    ref = rr.resize(yuv_ref.convert(Y, U, V, "420mpeg2", "709", False, True), 15, 27)
    assert np.array_equal(small.cpu().numpy(), ref), _first_difference(small.cpu().numpy(), ref)
    assert torch.equal(y4m.decode(data, gpu_device, matrix="auto"), whole)                       # 30 rows: 601
    with pytest.raises(ValueError, match="frame 4 is incomplete"):
        y4m.decode(data[:-7], gpu_device, chunk=2, fused=fused)


def test_read_video_on_a_y4m_downscales_by_the_front_ends_rule(gpu_device, tmp_path):
    data, _, (Y, U, V) = yc.case(96, 54, "420jpeg", F=4, seed=6, fps=(24, 1))
    path = tmp_path / "clip.y4m"
    path.write_bytes(data)
    assert frontend.target_size(96, 54, max_w=48) == (48, 27)
    want = rr.resize(yuv_ref.convert(Y, U, V, "420jpeg"), 27, 48)
    got, fps = frontend.read_video(str(path), gpu_device, max_w=48)
    assert got.shape == (4, 27, 48, 3) and got.is_cuda and fps == 24.0
    assert np.array_equal(got.cpu().numpy(), want), _first_difference(got.cpu().numpy(), want)
    again, _ = frontend.read_video(y4m.Reader(str(path)), gpu_device, max_w=48, bgr=True, matrix="709")
    assert np.array_equal(again.cpu().numpy(), rr.resize(yuv_ref.convert(Y, U, V, "420jpeg", "709", False, True), 27, 48))
    same, _ = frontend.read_video(str(path), gpu_device)                                          # below both limits: no resize
    assert np.array_equal(same.cpu().numpy(), yuv_ref.convert(Y, U, V, "420jpeg"))
    folder = tmp_path / "frames"
    n, (w, h), fps = frontend.prepare(str(path), str(folder), device=gpu_device, max_w=48)
    assert (n, w, h, fps) == (4, 48, 27, 24.0) and sorted(os.listdir(folder)) == [f"{i:09d}.jpg" for i in range(4)] + ["fps.txt"]


# ---- the Predictor on a YUV4MPEG2 file ----------------------------------------------------------------------------------------
def test_predictor_on_a_y4m_with_a_tracking_sidecar(gpu_device, tmp_path, monkeypatch):
    """Six 320x180 frames: the scores are those of score_frames on the tensor y4m.decode returns."""
    monkeypatch.setitem(sys.modules, "cv2", None)
    monkeypatch.setitem(sys.modules, "multi_person_tracker", None)
    W, H, frames = 320, 180, 6
    rng = np.random.default_rng(0)
    yy, xx = np.mgrid[0:H, 0:W]
    Y = np.stack([((xx + 3 * k + yy) % 256) for k in range(frames)]).astype(np.uint8)
    U = rng.integers(96, 160, (frames, H // 2, W // 2), dtype=np.uint8)
    V = rng.integers(96, 160, (frames, H // 2, W // 2), dtype=np.uint8)
    clip = tmp_path / "clip.y4m"
    y4m.write(clip, Y, U, V, fps=(24, 1), chroma="420mpeg2")
    track_frames = [0, 1, 2, 4, 5]
    track = {3: {"bbox": np.stack([np.array([150 + 4 * i, 90 - i, 70, 130], np.float32) for i in range(len(track_frames))]),
                 "frames": np.array(track_frames)}}
    with open(tmp_path / "clip.tracking.pkl", "wb") as f:
        pickle.dump(track, f)
    (tmp_path / "info.json").write_text(json.dumps(synth.EXAMPLE_INFO))
    model = hmr()
    model.load_state_dict(synth.hmr_state_dict(seed=1), strict=False)
    smpl = SMPL(models={"neutral": synth.smpl_model(V=6890, seed=2)}, device=gpu_device)
    args = types.SimpleNamespace(gpu="0", type="REBA,RULA", debug=False, debug_joints="", debug_frame=-1)
    pred = base.Predictor(args, spin_model=model, smpl_model=smpl, batch_size=4)
    assert pred.video_decoder == "" and cfg.DATASET.yuv_matrix == "601"
    out = pred(str(clip), str(tmp_path / "info.json"), str(tmp_path / "out"))
    assert out["frames"].tolist() == track_frames and out["fps"] == 24.0
    decoded = y4m.decode(str(clip), gpu_device)
    assert np.array_equal(decoded.cpu().numpy(), yuv_ref.convert(Y, U, V, "420mpeg2"))
    want = pred.score_frames(decoded, track, synth.EXAMPLE_INFO)
    for k in ("result", "joint_cam", "frames"):
        assert np.array_equal(np.asarray(out[k]), np.asarray(want[k])), k
    for t in ("reba", "rula"):
        np.testing.assert_array_equal(np.asarray(out[t][0], np.float64), np.asarray(want[t][0], np.float64), err_msg=t)
        for part in (1, 2):
            assert np.array_equal(np.asarray(out[t][part]), np.asarray(want[t][part])), (t, part)
