"""The PNG encoder on the GPU: every byte of every case against the contract's restatement (tests/png_enc_ref.py), every file
back through zlib + tests/png_ref.py and through this package's own decoder, the slots' bounds inside guard-band arenas, the
capacity rule, argument errors, determinism, graph capture, and the Predictor writing PNG frames with the gpu_video_codec knob."""
import io
import sys
import zlib

import numpy as np
import pytest
import torch

import guard_band as gb
import png_enc_cases as ec
import png_enc_ref as ref
import png_ref
from poserisk_release_amd import _lib, png, video
from test_jpeg_encode_gpu import _clip, _predictor

pytestmark = pytest.mark.gpu


def _first_difference(got, want):
    n = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
    return f"{len(got)} bytes for {len(want)}, the first difference at byte {n}"


def _groups():
    """The cases by (H, W, filter, mode): a group is one call."""
    groups = {}
    for c in ec.cases():
        groups.setdefault((*c["px"].shape[:2], c["filter"], c["mode"]), []).append(c)
    return groups


@pytest.mark.parametrize("bgr", [False, True])
def test_every_case_is_byte_identical_to_the_reference_and_decodes_to_its_pixels(gpu_device, bgr):
    groups = _groups()
    assert max(len(g) for g in groups.values()) >= 3            # several frames of different content in one call
    for (H, W, filt, mode), cases in groups.items():
        src = np.stack([c["px"][..., ::-1] if bgr else c["px"] for c in cases])
        buf, nbytes, status = png.encode_frames(torch.from_numpy(np.ascontiguousarray(src)).to(gpu_device), filter=filt, mode=mode, bgr=bgr)
        assert status.cpu().tolist() == [0] * len(cases)
        files = png.download_files(buf, nbytes)
        for c, data in zip(cases, files):
            want = ec.reference(c["name"])[0]
            assert data == want, f"{c['name']} bgr={bgr}: " + _first_difference(data, want)
            st, un = png_ref.unfilter(zlib.decompress(ref.idat_payload(data)[0]), H, W, 3)
            assert st == 0 and np.array_equal(un.reshape(H, W, 3), c["px"]), c["name"]
        back, dst = png.decode_files(files, gpu_device, bgr=bgr)
        assert dst.cpu().tolist() == [0] * len(cases), (H, W, filt, mode)
        assert np.array_equal(back.cpu().numpy(), src), (H, W, filt, mode)


def _smooth_noise_batch():
    smooth, noise = ec.smooth(160, 90), ec.noise(160, 90)
    batch = [smooth, noise, smooth[::-1].copy(), noise[:, ::-1].copy(), smooth]
    return batch, [ref.encode(f) for f in batch]


def test_a_slot_one_byte_short_gets_overflow_and_its_neighbours_stay_exact(gpu_device):
    batch, want = _smooth_noise_batch()
    cap = len(want[1]) - 1                                      # one byte short of frame 1's file; frame 3 has the same size
    assert len(want[3]) == len(want[1]) and max(len(want[i]) for i in (0, 2, 4)) < cap
    big, out = gb.arena((5, cap), torch.uint8, gpu_device, gb.CANARY_U8)
    nbytes, status = (torch.full((5,), -7, dtype=torch.int32, device=gpu_device) for _ in range(2))
    png.encode_frames(torch.from_numpy(np.stack(batch)).to(gpu_device), capacity=cap, out=(out, nbytes, status))
    torch.cuda.synchronize()
    gb.assert_guards_intact(big, out, "out")
    assert status.cpu().tolist() == [0, png.ENC_ST_OVERFLOW, 0, png.ENC_ST_OVERFLOW, 0]
    assert nbytes.cpu().tolist() == [len(want[0]), 0, len(want[2]), 0, len(want[4])]
    got = out.cpu().numpy()
    for i in (0, 2, 4):
        assert got[i, :len(want[i])].tobytes() == want[i] and (got[i, len(want[i]):] == gb.CANARY_U8).all()
    assert (got[[1, 3]] == gb.CANARY_U8).all()                  # nothing at all in the slots of the frames that did not fit
    exact = png.encode_frames(torch.from_numpy(np.stack(batch[1:2])).to(gpu_device), capacity=cap + 1)
    assert exact[2].cpu().tolist() == [0] and png.download_files(exact[0], exact[1])[0] == want[1]


def test_every_tensor_stays_inside_its_guard_bands(gpu_device):
    """683 x 9 (two segments, the boundary inside a row) with an odd slot size, so that slots start at every alignment."""
    px = [ec.smooth(683, 9), ec.crossing(), ec.noise(683, 9)]
    want = [ref.encode(p) for p in px]
    F, H, W, cap = 3, 9, 683, ref.bound(9, 683) + 1
    frames_arena, frames = gb.guarded_input(torch.from_numpy(np.stack(px)), gpu_device)
    plan_host = torch.from_numpy(np.frombuffer(png.encode_plan("adaptive", "rle", H, W).tobytes(), np.uint8).copy())
    plan_arena, plan = gb.guarded_input(plan_host, gpu_device)
    need = png.encode_workspace_bytes(F, H, W)
    arenas = {n: gb.arena(shape, dtype, gpu_device, gb.canary(dtype)) for n, shape, dtype in
              (("out", (F, cap), torch.uint8), ("nbytes", (F,), torch.int32), ("status", (F,), torch.int32),
               ("workspace", (need,), torch.uint8))}
    out, nbytes, status, ws = (arenas[n][1] for n in ("out", "nbytes", "status", "workspace"))
    assert ws.data_ptr() % 16 == 0
    before, plan_before = frames.clone(), plan.clone()
    args = _lib.PngEncArgs(frames.data_ptr(), plan.data_ptr(), out.data_ptr(), nbytes.data_ptr(), status.data_ptr(), cap, F, H, W,
                           5, 1, 0)
    _lib.check(_lib.load().pr_png_encode(args, ws.data_ptr(), need, torch.cuda.current_stream().cuda_stream), "pr_png_encode")
    torch.cuda.synchronize()
    for name, (big, view) in arenas.items():
        gb.assert_guards_intact(big, view, name)
    gb.assert_guards_intact(frames_arena, frames, "frames")
    gb.assert_guards_intact(plan_arena, plan, "plan")
    assert torch.equal(frames, before) and torch.equal(plan, plan_before)
    assert status.cpu().tolist() == [0] * F and nbytes.cpu().tolist() == [len(w) for w in want]
    got = out.cpu().numpy()
    for i in range(F):
        assert got[i, :len(want[i])].tobytes() == want[i]
        assert (got[i, len(want[i]):] == gb.CANARY_U8).all(), f"slot {i}: bytes written behind nbytes"


def test_argument_errors_by_name_and_an_empty_call(gpu_device):
    lib = _lib.load()
    F, H, W = 2, 16, 21
    frames = torch.zeros((F, H, W, 3), dtype=torch.uint8, device=gpu_device)
    plan = torch.from_numpy(np.frombuffer(png.encode_plan(5, 1, H, W).tobytes(), np.uint8).copy()).to(gpu_device)
    cap, need = png.encode_bound(H, W), png.encode_workspace_bytes(F, H, W)
    out = torch.full((F, cap), 7, dtype=torch.uint8, device=gpu_device)
    nbytes, status = (torch.full((F,), -7, dtype=torch.int32, device=gpu_device) for _ in range(2))
    ws = torch.empty(need + 16, dtype=torch.uint8, device=gpu_device)
    stream = torch.cuda.current_stream().cuda_stream

    def call(ws_ptr=None, ws_bytes=None, **over):
        v = dict(frames=frames.data_ptr(), plan=plan.data_ptr(), out=out.data_ptr(), nbytes=nbytes.data_ptr(), status=status.data_ptr(),
                 capacity=cap, F=F, H=H, W=W, filter=5, mode=1, bgr=0)
        v.update(over)
        rc = lib.pr_png_encode(_lib.PngEncArgs(**v), ws.data_ptr() if ws_ptr is None else ws_ptr, need if ws_bytes is None else ws_bytes, stream)
        return rc, lib.pr_last_error().decode()
    for over, word in ((dict(frames=None), "null frames"), (dict(plan=None), "null plan"), (dict(out=None), "null out"),
                       (dict(nbytes=None), "null nbytes"), (dict(status=None), "null status"), (dict(F=-1), "F = -1"),
                       (dict(F=70000), "65535"), (dict(H=0), "sizes 1.."), (dict(W=4097), "sizes 1.."), (dict(filter=6), "filter 6"),
                       (dict(mode=2), "mode 2"), (dict(capacity=-1), "capacity"), (dict(capacity=1 << 31), "capacity"),
                       (dict(ws_ptr=0), "null workspace"), (dict(ws_ptr=ws.data_ptr() + 1), "16-byte aligned"),
                       (dict(ws_bytes=need - 1), "needed")):
        rc, msg = call(**over)
        assert rc == -1 and word in msg, (over, rc, msg)       # PR_ERR_INVALID
    assert lib.pr_png_encode(None, ws.data_ptr(), need, stream) == -1
    torch.cuda.synchronize()
    assert (out == 7).all() and (nbytes == -7).all() and (status == -7).all()      # no device work happened
    assert call(F=0, frames=None, out=None)[0] == 0            # F = 0: PR_OK, nothing looked at
    empty = png.encode_frames(frames[:0])
    assert tuple(empty[0].shape) == (0, cap) and png.download_files(empty[0], empty[1]) == []
    with pytest.raises(ValueError, match="filter"):
        png.encode_frames(frames, filter="best")
    with pytest.raises(ValueError, match="mode"):
        png.encode_frames(frames, mode="fixed")
    with pytest.raises(ValueError, match="workspace"):
        png.encode_frames(frames, workspace=ws[:64])
    with pytest.raises(_lib.PoseRiskHipError, match="GPU only"):
        png.encode_frames(frames.cpu())


def test_the_same_call_twice_and_a_captured_graph_give_identical_bytes(gpu_device):
    batch, want = _smooth_noise_batch()
    F, cap = len(batch), ref.bound(90, 160)
    frames = torch.from_numpy(np.stack(batch)).to(gpu_device)
    ws = torch.empty(png.encode_workspace_bytes(F, 90, 160), dtype=torch.uint8, device=gpu_device)
    outs = [(torch.zeros((F, cap), dtype=torch.uint8, device=gpu_device), torch.zeros(F, dtype=torch.int32, device=gpu_device),
             torch.zeros(F, dtype=torch.int32, device=gpu_device)) for _ in range(3)]
    for o in outs[:2]:
        png.encode_frames(frames, out=o, workspace=ws)          # also uploads the plan, outside the capture
    torch.cuda.synchronize()
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert png.download_files(outs[0][0], outs[0][1]) == want
    side = torch.cuda.Stream(gpu_device)
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            png.encode_frames(frames, out=outs[2], workspace=ws)
    for _ in range(2):
        outs[2][0].zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(outs[2][1], outs[0][1]) and not outs[2][2].any()
        assert png.download_files(outs[2][0], outs[2][1]) == want


# ---- end to end: Predictor.__call__ with gpu_video_codec 'png' ------------------------------------------------------------------
def _read_png(path):
    blob = open(path, "rb").read()
    pst, dst, px = png_ref.decode(blob) if len(blob) < 1 << 16 else (0, 0, None)
    if px is None:                                              # a large file: zlib inflates, the reference unfilters
        fr = png_ref.parse(blob)
        st, un = png_ref.unfilter(zlib.decompress(ref.idat_payload(blob)[0]), fr["height"], fr["width"], 3)
        assert fr["status"] == 0 and fr["color_type"] == 2 and st == 0
        px = un.reshape(fr["height"], fr["width"], 3)
    assert pst == 0 and dst == 0
    return px


@pytest.mark.parametrize("render_mesh", [False, True])
def test_predictor_writes_gpu_encoded_png_frames(gpu_device, tmp_path, monkeypatch, render_mesh):
    monkeypatch.setitem(sys.modules, "cv2", None)              # with or without cv2 the files are the GPU's
    frames, src = _clip(tmp_path)
    pred = _predictor(gpu_device, gpu_video=True, video_codec="png", render_mesh=render_mesh)
    assert pred.gpu_video_codec == "png"
    seen = []
    real = png.encode_frames
    monkeypatch.setattr(png, "encode_frames", lambda *a, **k: (seen.append(int(a[0].shape[0])), real(*a, **k))[1])
    out = pred(src, "", str(tmp_path / "out"))
    assert sum(seen) >= 9                                      # the files came from the device encoder
    vdir = tmp_path / "out" / "REBA_video"
    assert sorted(p.name for p in vdir.iterdir()) == ['{0:09d}.png'.format(i) for i in range(9)]
    assert not any(p.suffix in (".avi", ".mp4") for p in (tmp_path / "out").iterdir())
    _, scores, logs, _ = out["reba"]
    draw = video.draw_list("REBA", 9, out['bboxes'], (0, out['frames'], 9), scores, pred.reba.eval_items, logs, 540)
    dev = torch.from_numpy(frames).to(gpu_device)
    overlay = None
    if render_mesh:
        mdir = tmp_path / "out" / "REBA_mesh"
        numbers = [1, 2, 3, 4, 5, 6, 8]
        assert sorted(p.name for p in mdir.iterdir()) == ['{0:09d}.png'.format(i) for i in numbers]
        parts = list(pred.render_overlay(out, dev, "REBA", False))
        over = {int(f): im for fr, img in parts for f, im in zip(fr, img)}
        assert sorted(over) == numbers
        for f in numbers:
            assert np.array_equal(_read_png(mdir / '{0:09d}.png'.format(f)), over[f].cpu().numpy()), f"mesh frame {f}"

        def overlay(lo, hi):                                   # the overlaid track frames of [lo, hi), as write_gpu_video hands them on
            sel = [f for f in numbers if lo <= f < hi]
            return (np.array(sel), torch.stack([over[f] for f in sel])) if sel else ([], None)
    want = torch.cat(list(video.annotated_frames(dev, draw, 4, overlay=overlay))).cpu().numpy()
    assert want.shape == (9, 540, 1000, 3)
    for i in range(9):
        assert np.array_equal(_read_png(vdir / '{0:09d}.png'.format(i)), want[i]), f"video frame {i}"
    if render_mesh:                                            # and the overlay is in them: they differ from the plain canvases
        plain = torch.cat(list(video.annotated_frames(dev, draw, 4))).cpu().numpy()
        assert all((want[f] != plain[f]).any() for f in numbers) and np.array_equal(want[0], plain[0])


def test_an_unknown_codec_still_raises_by_name(gpu_device):
    with pytest.raises(ValueError, match="h264"):
        _predictor(gpu_device, gpu_video=True, video_codec="h264")
