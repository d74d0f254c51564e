"""The JPEG encoder on the GPU: every byte against Pillow's files (tests/golden/jpeg_encode.npz) and against the numpy
restatement of the contract (tests/jpeg_enc_ref.py), the slots' bounds inside guard-band arenas, the capacity rule, and the
Predictor writing Motion-JPEG AVI files with the gpu_video_codec knob.  Needs neither Pillow nor cv2.

The encoder's parameters (quality, sampling, restart interval) belong to a call, not to a frame, so the golden cases, which vary
them, take one call per (size, parameters) group rather than one per size."""
import functools
import pickle
import sys
import types

import numpy as np
import pytest
import torch

import guard_band as gb
import jpeg_enc_cases as ec
import jpeg_enc_ref as er
import jpeg_ref as jr
import riff_reader
from poserisk_release_amd import jpeg, synth, video

pytestmark = pytest.mark.gpu


def _files(buf, nbytes, status):
    assert status.cpu().tolist() == [0] * len(status), status.cpu().tolist()
    return jpeg.download_files(buf, nbytes)


def _first_difference(got, want):
    n = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
    return f"{len(got)} bytes for {len(want)}, the first difference at byte {n}"


@pytest.mark.parametrize("bgr", [False, True])
def test_every_small_golden_case_is_byte_identical_to_pillows_file(gpu_device, bgr):
    groups = {}
    for c in ec.small_cases():
        groups.setdefault((c["src"].shape[:2], c["quality"], c["subsampling"], c["restart_interval"]), []).append(c)
    assert len({k[0] for k in groups}) == 6 and sum(len(g) for g in groups.values()) >= 50
    for ((H, W), quality, samp, ri), cases in groups.items():
        assert ri in (0, -1, 3)
        src = np.stack([c["src"][..., ::-1] if bgr else c["src"] for c in cases])
        frames = torch.from_numpy(np.ascontiguousarray(src)).to(gpu_device)
        if ri == 3:                                             # encode_frames offers rows or none: the general interval by the binding
            got = _files(*_encode_with_interval(frames, quality, samp, 3, bgr))
        else:
            got = _files(*jpeg.encode_frames(frames, quality=quality, subsampling=samp, restart_rows=1 if ri else 0, bgr=bgr,
                                             capacity=jpeg.encode_bound(H, W, samp, ri)))   # noise at quality 100 passes the default
        for c, data in zip(cases, got):
            assert data == c["data"], f"{c['name']} bgr={bgr}: " + _first_difference(data, c["data"])


def _encode_with_interval(frames, quality, samp, ri, bgr, capacity=None):
    """pr_jpeg_encode with a restart interval given in MCUs, which encode_frames does not offer."""
    from poserisk_release_amd import _lib
    lib, (F, H, W, _) = _lib.load(), frames.shape
    hs, vs = jpeg.SUBSAMPLING[samp]
    plan = torch.from_numpy(np.frombuffer(jpeg.encode_plan(quality, samp, ri, H, W).tobytes(), np.uint8).copy()).to(frames.device)
    cap = capacity if capacity is not None else jpeg.encode_bound(H, W, samp, ri)
    buf = torch.empty((F, cap), dtype=torch.uint8, device=frames.device)
    nbytes, status = (torch.empty(F, dtype=torch.int32, device=frames.device) for _ in range(2))
    ws = torch.empty(lib.pr_jpeg_encode_workspace_bytes(F, H, W, hs, vs, ri, cap), dtype=torch.uint8, device=frames.device)
    args = _lib.JpegEncArgs(frames.data_ptr(), plan.data_ptr(), buf.data_ptr(), nbytes.data_ptr(), status.data_ptr(), cap, F, H, W,
                            hs, vs, ri, int(bgr))
    _lib.check(lib.pr_jpeg_encode(args, ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream), "pr_jpeg_encode")
    torch.cuda.synchronize()
    return buf, nbytes, status


def test_mixed_content_in_one_call_at_every_small_size(gpu_device):
    """The golden test's calls hold the few cases that share all parameters, often one frame.  Here every size takes one call
    of five frames of mixed content (smooth, noise, both flipped, smooth again) against the numpy restatement, with a
    caller-owned workspace that the next size reuses."""
    by_size = {}
    for c in ec.small_cases():
        kind = "noise" if "_noise_" in c["name"] else "smooth"
        by_size.setdefault(c["src"].shape[:2], {}).setdefault(kind, c["src"])
    assert len(by_size) == 6 and all(set(v) == {"smooth", "noise"} for v in by_size.values())
    params = [(75, "4:2:0", 1), (100, "4:2:2", 0), (30, "4:4:4", 1), (90, "4:2:0", 0), (100, "4:2:0", 1), (90, "4:2:2", 1)]
    need = max(jpeg.encode_workspace_bytes(5, H, W, samp, rows, jpeg.encode_bound(H, W, samp, -rows))
               for (H, W), (_, samp, rows) in zip(sorted(by_size), params))
    ws = torch.empty(need, dtype=torch.uint8, device=gpu_device)
    for (H, W), (quality, samp, rows) in zip(sorted(by_size), params):
        smooth, noise = by_size[(H, W)]["smooth"], by_size[(H, W)]["noise"]
        batch = [smooth, noise, smooth[::-1].copy(), noise[:, ::-1].copy(), smooth]
        want = [er.encode(f, quality, samp, -rows) for f in batch[:4]]
        got = _files(*jpeg.encode_frames(torch.from_numpy(np.stack(batch)).to(gpu_device), quality=quality, subsampling=samp,
                                         restart_rows=rows, capacity=jpeg.encode_bound(H, W, samp, -rows), workspace=ws))
        for i, data in enumerate(got):
            assert data == want[i % 4], f"{W}x{H} {samp} q{quality} frame {i}: " + _first_difference(data, want[i % 4])
    with pytest.raises(ValueError, match="workspace"):
        jpeg.encode_frames(torch.zeros((1, 16, 16, 3), dtype=torch.uint8, device=gpu_device), workspace=ws[:64])


@functools.lru_cache(maxsize=None)
def _canvas_rolls():
    """The golden 450x1000 source rolled by 11 i columns, i = 0..3, and the reference encoder's bytes of each (computed once)."""
    c = ec.canvas_case()
    rolls = [np.roll(c["src"], 11 * i, axis=1) for i in range(4)]
    want = [er.encode(r, 90, "4:2:0", -1) for r in rolls]
    assert want[0] == c["data"]                                # roll 0 is Pillow's file
    return rolls, want


def test_64_canvases_in_one_call_equal_the_reference_at_every_position(gpu_device):
    rolls, want = _canvas_rolls()
    order = np.arange(64) % 4
    order[4:] = np.random.default_rng(64).integers(0, 4, 60)
    frames = torch.from_numpy(np.stack([rolls[i] for i in order])).to(gpu_device)
    got = _files(*jpeg.encode_frames(frames, quality=90, subsampling="4:2:0", restart_rows=1))
    assert len(got) == 64
    for pos, i in enumerate(order):
        assert got[pos] == want[i], f"position {pos} (roll {i}): " + _first_difference(got[pos], want[i])
    for i in range(4):                                         # and alone
        one = _files(*jpeg.encode_frames(frames[i:i + 1].clone(), quality=90))
        assert one[0] == want[i], f"roll {i} alone: " + _first_difference(one[0], want[i])


def test_round_trip_through_the_decoder(gpu_device):
    cases = [c for c in ec.small_cases() if c["name"] in ("37x29_smooth_420_q75_row", "160x120_noise_420_q100_none",
                                                         "33x17_smooth_422_q90_row", "48x32_smooth_444_q100_row")]
    assert len(cases) == 4
    for c in cases:
        frames = torch.from_numpy(np.stack([c["src"], c["src"][::-1].copy()])).to(gpu_device)
        files = _files(*jpeg.encode_frames(frames, quality=c["quality"], subsampling=c["subsampling"],
                                           restart_rows=1 if c["restart_interval"] else 0,
                                           capacity=jpeg.encode_bound(*c["src"].shape[:2], c["subsampling"], c["restart_interval"])))
        back, status = jpeg.decode_files(files, gpu_device)
        assert status.cpu().tolist() == [0, 0], c["name"]
        for f, px in zip(files, back.cpu().numpy()):
            np.testing.assert_array_equal(px, jr.decode(f), err_msg=c["name"])


def test_outputs_stay_inside_their_guard_bands(gpu_device):
    rolls, want = _canvas_rolls()
    F, cap = 3, max(len(w) for w in want) + 1000
    frames_arena, frames = gb.guarded_input(torch.from_numpy(np.stack(rolls[:F])), gpu_device)     # fenced with 255
    arenas = {n: gb.arena(shape, dtype, gpu_device, gb.canary(dtype)) for n, shape, dtype in
              (("out", (F, cap), torch.uint8), ("nbytes", (F,), torch.int32), ("status", (F,), torch.int32))}
    before = frames.clone()
    buf, nbytes, status = jpeg.encode_frames(frames, quality=90, capacity=cap, out=tuple(arenas[n][1] for n in ("out", "nbytes", "status")))
    torch.cuda.synchronize()
    assert buf.data_ptr() == arenas["out"][1].data_ptr()
    for name, (big, view) in arenas.items():
        gb.assert_guards_intact(big, view, name)
    gb.assert_guards_intact(frames_arena, frames, "frames")
    assert torch.equal(frames, before)
    assert status.cpu().tolist() == [0] * F and nbytes.cpu().tolist() == [len(w) for w in want[:F]]
    got = buf.cpu().numpy()
    for i in range(F):
        assert got[i, :len(want[i])].tobytes() == want[i]
        assert (got[i, len(want[i]):] == gb.CANARY_U8).all(), f"slot {i}: bytes written behind nbytes"


def test_a_frame_that_does_not_fit_gets_overflow_and_its_neighbours_stay_exact(gpu_device):
    rng = np.random.default_rng(8)
    smooth = next(c for c in ec.small_cases() if c["name"].startswith("160x120_smooth"))["src"]
    noise = rng.integers(0, 256, smooth.shape, dtype=np.uint8)
    batch = [smooth, noise, smooth[::-1].copy(), noise[:, ::-1].copy(), smooth]
    want = [er.encode(f, 100, "4:2:0", -1) for f in batch]
    cap = max(len(want[0]), len(want[2])) + 64                 # from the CPU reference: the noise frames are certainly too long
    assert min(len(want[1]), len(want[3])) > cap + 1000
    big, out = gb.arena((5, cap), torch.uint8, gpu_device, gb.CANARY_U8)
    nbytes, status = (torch.full((5,), -7, dtype=torch.int32, device=gpu_device) for _ in range(2))
    jpeg.encode_frames(torch.from_numpy(np.stack(batch)).to(gpu_device), quality=100, capacity=cap, out=(out, nbytes, status))
    torch.cuda.synchronize()
    gb.assert_guards_intact(big, out, "out")
    assert status.cpu().tolist() == [0, jpeg.ENC_ST_OVERFLOW, 0, jpeg.ENC_ST_OVERFLOW, 0]
    assert nbytes.cpu().tolist() == [len(want[0]), 0, len(want[2]), 0, len(want[4])]
    got = out.cpu().numpy()
    for i in (0, 2, 4):
        assert got[i, :len(want[i])].tobytes() == want[i] and (got[i, len(want[i]):] == gb.CANARY_U8).all()
    assert (got[[1, 3]] == gb.CANARY_U8).all()                 # nothing at all in the slots of the frames that did not fit
    files = jpeg.download_files(out, nbytes)
    assert [len(f) for f in files] == nbytes.cpu().tolist() and files[2] == want[2]
    # the slot no file exceeds holds them
    full = _files(*jpeg.encode_frames(torch.from_numpy(np.stack(batch[1:2])).to(gpu_device), quality=100,
                                      capacity=jpeg.encode_bound(120, 160)))
    assert full[0] == want[1]


def test_the_call_is_ordered_by_its_stream_alone(gpu_device):
    """On a side stream, behind the copy that produces its input and in front of the copy that reads its output, with no
    synchronisation in between: the result alone says whether the call kept to the stream."""
    c = next(c for c in ec.small_cases() if c["name"] == "1000x50_smooth_420_q90_row")
    host = torch.from_numpy(np.stack([c["src"]] * 8)).pin_memory()
    side = torch.cuda.Stream(gpu_device)
    with torch.cuda.stream(side):
        frames = torch.zeros(host.shape, dtype=torch.uint8, device=gpu_device)
        frames.copy_(host, non_blocking=True)
        buf, nbytes, status = jpeg.encode_frames(frames, quality=90)
        got_n = nbytes.to("cpu", non_blocking=True)
        got = buf.to("cpu", non_blocking=True)
    side.synchronize()
    assert got_n.tolist() == [len(c["data"])] * 8 and not status.any()
    assert all(got[i, :len(c["data"])].numpy().tobytes() == c["data"] for i in range(8))


# ---- end to end: Predictor.__call__ with the gpu_video_codec knob -------------------------------------------------------------
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
    """The synthetic clip of tests/test_video_gpu.py: 9 frames of 320 x 240, a track over frames 1-6 and 8."""
    rng = np.random.default_rng(9)
    frames = rng.integers(0, 256, (9, 240, 320, 3), dtype=np.uint8)
    fr = [1, 2, 3, 4, 5, 6, 8]
    tr = {8: {'bbox': np.stack([np.array([160 + 3 * i, 120 - 2 * i, 90, 180], np.float32) for i in range(len(fr))]),
              'frames': np.array(fr)}}
    src = tmp_path / "clip"
    src.mkdir()
    np.save(src / "frames.npy", frames)
    with open(src / "tracking.pkl", "wb") as f:
        pickle.dump(tr, f)
    return frames, str(src)


def test_predictor_writes_motion_jpeg_without_cv2(gpu_device, tmp_path, monkeypatch):
    monkeypatch.setitem(sys.modules, "cv2", None)              # `import cv2` raises ImportError
    frames, src = _clip(tmp_path)
    pred = _predictor(gpu_device, gpu_video=True, video_codec="mjpeg")
    assert pred.gpu_video_codec == "mjpeg" and pred.gpu_video_quality == 90
    out = pred(src, "", str(tmp_path / "out"))
    names = sorted(p.name for p in (tmp_path / "out").iterdir())
    assert "REBA_video.avi" in names and "REBA_video" not in names and "REBA_video.mp4" not in names
    avi = riff_reader.read_avi(tmp_path / "out" / "REBA_video.avi")
    assert avi["count"] == avi["stream_count"] == len(avi["frames"]) == 9 and (avi["width"], avi["height"]) == (1000, 540)
    assert abs(avi["fps"] - float(out["fps"])) < 1e-3 and avi["handler"] == b"MJPG"
    _, scores, logs, _ = out["reba"]
    draw = video.draw_list("REBA", 9, out['bboxes'], (0, out['frames'], 9), scores, pred.reba.eval_items, logs, 540)
    lines, codes = video.pack_lines(draw.text)
    canvases = video.compose(torch.from_numpy(frames).to(gpu_device), None, draw.box, lines, codes)
    want_files = _files(*jpeg.encode_frames(canvases.contiguous(), quality=90))
    assert avi["frames"] == want_files
    got, st = jpeg.decode_files(avi["frames"], gpu_device)
    want, st2 = jpeg.decode_files(want_files, gpu_device)
    assert not st.any() and not st2.any() and torch.equal(got, want) and tuple(got.shape) == (9, 540, 1000, 3)


def test_predictor_writes_the_mesh_as_motion_jpeg_too(gpu_device, tmp_path, monkeypatch):
    monkeypatch.setitem(sys.modules, "cv2", None)
    frames, src = _clip(tmp_path)
    pred = _predictor(gpu_device, gpu_video=True, render_mesh=True, video_codec="mjpeg")
    out = pred(src, "", str(tmp_path / "out"))
    names = sorted(p.name for p in (tmp_path / "out").iterdir())
    assert "REBA_video.avi" in names and "REBA_mesh.avi" in names and "REBA_mesh" not in names
    mesh = riff_reader.read_avi(tmp_path / "out" / "REBA_mesh.avi")
    assert mesh["count"] == len(mesh["frames"]) == len(out["frames"]) == 7 and (mesh["width"], mesh["height"]) == (320, 240)
    px, st = jpeg.decode_files(mesh["frames"], gpu_device)
    assert not st.any() and tuple(px.shape) == (7, 240, 320, 3)
    assert riff_reader.read_avi(tmp_path / "out" / "REBA_video.avi")["count"] == 9


def test_without_the_codec_knob_the_outputs_are_the_earlier_ones(gpu_device, tmp_path, monkeypatch):
    monkeypatch.setitem(sys.modules, "cv2", None)
    frames, src = _clip(tmp_path)
    pred = _predictor(gpu_device, gpu_video=True, render_mesh=True)
    assert pred.gpu_video_codec == ""
    pred(src, "", str(tmp_path / "out"))
    names = sorted(p.name for p in (tmp_path / "out").iterdir())
    assert not any(n.endswith(".avi") for n in names), names
    assert (tmp_path / "out" / "REBA_video").is_dir() and (tmp_path / "out" / "REBA_mesh").is_dir()
    assert sorted(p.name for p in (tmp_path / "out" / "REBA_video").iterdir()) == ['{0:09d}.png'.format(i) for i in range(9)]
    assert sorted(p.name for p in (tmp_path / "out" / "REBA_mesh").iterdir()) == ['{0:09d}.png'.format(i) for i in (1, 2, 3, 4, 5, 6, 8)]
    with pytest.raises(ValueError, match="h264"):
        _predictor(gpu_device, gpu_video=True, video_codec="h264")
