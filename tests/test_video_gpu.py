"""GPU: the annotated score video's compositor (csrc/compose.hip, pr_compose_video) against the numpy restatement of its
contract (tests/video_ref.py), every byte of every checked canvas; batch independence; hipGraph capture; and end to end
through Predictor.__call__ with the gpu_video knob."""
import pickle
import sys
import types

import numpy as np
import pytest
import torch

import video_ref as vr
from poserisk_release_amd import _lib, render, synth, video

pytestmark = pytest.mark.gpu

N_FRAMES = 5
BOX_RGB = (17, 250, 99)


def _random_atlas(seed=5):
    """A coverage atlas of noise in three odd sizes: every pixel of every cell matters, which a real font's mostly empty cells
    would not show."""
    rng = np.random.default_rng(seed)
    cov = rng.integers(0, 256, (3, 96, 11, 7), dtype=np.uint8)
    cov[rng.random(cov.shape) < 0.2] = 0
    cov[rng.random(cov.shape) < 0.2] = 255
    return video.Atlas(cov, (7, 5, 3), (9, 4, 0))


def _frames(H, W, seed):
    return np.random.default_rng(seed).integers(0, 256, (N_FRAMES, H, W, 3), dtype=np.uint8)


def _boxes(N, H, W, rng):
    """Per canvas, in turn: inside, partly off the frame, wholly off, thinner than 4 px, none, random."""
    box = np.zeros((N, 4), np.int32)
    for n in range(N):
        kind = n % 6
        if kind == 0:
            x0, y0 = rng.integers(2, W // 2), rng.integers(2, H // 2)
            box[n] = (x0, y0, x0 + rng.integers(4, W // 2 - 2), y0 + rng.integers(4, H // 2 - 2))
        elif kind == 1:
            box[n] = (-rng.integers(1, 30), rng.integers(0, H // 2), rng.integers(W // 2, W + 30), H + rng.integers(0, 9) - 3)
        elif kind == 2:
            box[n] = (W + 5, H + 7, W + 60, H + 90)
        elif kind == 3:
            x0, y0 = rng.integers(0, W - 3), rng.integers(0, H - 3)
            box[n] = (x0, y0, x0 + rng.integers(0, 4), y0 + rng.integers(0, 4))
        elif kind == 4:
            box[n] = video.NO_BOX
        else:
            a, b = np.sort(rng.integers(-20, W + 20, 2)), np.sort(rng.integers(-20, H + 20, 2))
            box[n] = (a[0], b[0], a[1], b[1])
    return box


def _lines(N, L, C, atlas, dst_h, dst_w, panel_w, rng):
    """L lines per canvas over the panel: overlapping (16 lines of up to C cells in 280 px), starting left of the panel and
    running over the canvas's right edge, above the top and below the bottom, with size classes and codes outside their ranges,
    empty lines and lengths beyond C."""
    S, _, CH, CW = atlas.cov.shape
    lines = np.zeros((N, L, 5), np.int32)
    lines[..., 0] = rng.integers(dst_w - 60, dst_w + panel_w + 10, (N, L))
    lines[..., 1] = rng.integers(-5, dst_h + CH + 5, (N, L))
    lines[..., 2] = rng.integers(0, S, (N, L))
    lines[..., 3] = rng.integers(1, C + 1, (N, L))
    lines[..., 4] = rng.integers(0, 1 << 24, (N, L))
    lines[:, 1::7, 0] = dst_w + panel_w - 3 * CW                 # clipped at the right edge
    lines[:, 2::7, 1] = dst_h + 2                                 # clipped at the bottom edge
    lines[:, 3::7, 2] = rng.choice([-1, S, 7], (N, len(range(3, L, 7))))      # no such size class
    lines[:, 4::7, 3] = rng.choice([0, -3], (N, len(range(4, L, 7))))         # empty
    lines[:, 5::7, 3] = C + 9                                     # longer than the row of codes: clamped to C
    text = rng.integers(32, 128, (N, L, C), dtype=np.uint8)
    wild = rng.random((N, L, C)) < 0.15
    text[wild] = rng.integers(0, 256, int(wild.sum()), dtype=np.uint8)        # codes outside 32..127 draw nothing
    return lines, text


def _case(H, W, N, atlas, seed, L=16, C=12):
    rng = np.random.default_rng(seed)
    frames = _frames(H, W, seed)
    dst_h, dst_w, panel_w = video.canvas_size(H, W)
    src_idx = rng.integers(0, N_FRAMES, N).astype(np.int32)       # repeated as soon as N > 5
    if N >= 7:
        src_idx[3], src_idx[N - 1] = N_FRAMES, -1                 # out of range, either side
    box = _boxes(N, H, W, rng)
    lines, text = _lines(N, L, C, atlas, dst_h, dst_w, panel_w, rng)
    return dict(frames=frames, src_idx=src_idx, box=box, lines=lines, text=text, atlas=atlas, dst_h=dst_h, dst_w=dst_w,
                panel_w=panel_w)


def _run(case, dev, sel=slice(None), **kw):
    fr = case["frames"] if isinstance(case["frames"], torch.Tensor) else torch.from_numpy(case["frames"]).to(dev)
    return video.compose(fr, case["src_idx"][sel], case["box"][sel], case["lines"][sel], case["text"][sel], case["atlas"],
                         case["dst_h"], case["dst_w"], case["panel_w"], box_rgb=BOX_RGB, **kw)


def _reference(case, canvases):
    a = case["atlas"]
    return vr.compose(case["frames"], case["src_idx"], case["box"], case["lines"], case["text"], np.asarray(a.cov), a.adv, a.ascent,
                      case["dst_h"], case["dst_w"], case["panel_w"], BOX_RGB, canvases=canvases)


def _check_canvases(N):
    return list(range(N)) if N <= 7 else sorted(set(range(0, N, 9)) | {3, N - 1})


@pytest.mark.parametrize("font", ["random", "dejavu"])
@pytest.mark.parametrize("N", [1, 7, 64])
@pytest.mark.parametrize("H,W", [(450, 800), (1080, 1920), (37, 53), (480, 640)])
def test_compose_matches_reference_bit_for_bit(gpu_device, H, W, N, font):
    atlas = _random_atlas() if font == "random" else video.font_atlas()
    case = _case(H, W, N, atlas, seed=H + N)
    out, st = _run(case, gpu_device, return_status=True)
    out, st = out.cpu().numpy(), st.cpu().numpy()
    assert out.shape == (N, case["dst_h"], case["dst_w"] + case["panel_w"], 3)
    check = _check_canvases(N)
    want, want_st = _reference(case, check)
    np.testing.assert_array_equal(st, want_st)
    assert (N < 7) or st.tolist().count(1) == 2
    drawn = boxed = 0
    for n in check:
        bad = np.argwhere(out[n] != want[n])
        assert bad.size == 0, f"canvas {n}: {len(bad)} bytes differ, first (row, col, channel) {bad[0].tolist()}: " \
                              f"{out[n][tuple(bad[0])]} != {want[n][tuple(bad[0])]}"
        if st[n]:                                                  # no such frame: image region zero, panel intact
            assert not out[n, :, :case["dst_w"]].any()
        drawn += int(out[n, :, case["dst_w"]:].any())
        f = int(case["src_idx"][n])
        if 0 <= f < N_FRAMES and n % 6 in (0, 1, 3):               # the box changed the image
            boxed += int((out[n, :, :case["dst_w"]] != vr.area_resample(case["frames"][f], case["dst_h"], case["dst_w"])).any())
    assert drawn == len(check) and boxed > 0


@pytest.mark.parametrize("boxed", [True, False], ids=["box", "no_box"])
def test_sixteen_lines_on_a_ragged_upsampled_canvas(gpu_device, boxed):
    """37 x 53 frames to 40 x 31: 3 W = 111 is no multiple of 16, dst_h no multiple of the band's 8 rows, two taps per column;
    PR_VIDEO_MAX_LINES lines, with a box and with box=None."""
    H, W, N, L = 53, 37, 7, 16
    case = dict(_case(H, W, N, _random_atlas(), seed=3, L=L), dst_h=31, dst_w=40, panel_w=23)
    case["lines"], case["text"] = _lines(N, L, 12, case["atlas"], 31, 40, 23, np.random.default_rng(4))
    if not boxed:
        case["box"] = np.tile(np.array(video.NO_BOX, np.int32), (N, 1))
    fr = torch.from_numpy(case["frames"]).to(gpu_device)
    out, st = video.compose(fr, case["src_idx"], case["box"] if boxed else None, case["lines"], case["text"], case["atlas"], 31, 40, 23,
                            box_rgb=BOX_RGB, return_status=True)
    want, want_st = _reference(case, list(range(N)))
    assert out.shape == (N, 31, 63, 3) and np.array_equal(st.cpu().numpy(), want_st) and st.tolist().count(1) == 2
    bad = np.argwhere(out.cpu().numpy() != want)
    assert bad.size == 0, f"{len(bad)} bytes differ, first (canvas, row, col, channel) {bad[0].tolist()}"
    assert want[:, :, 40:].any() and want[:, :, :40].any()
    plain = np.stack([vr.area_resample(case["frames"][f], 31, 40) if 0 <= f < N_FRAMES else np.zeros((31, 40, 3), np.uint8)
                      for f in case["src_idx"]])
    assert (want[:, :, :40] != plain).any() == boxed                     # the box, in BOX_RGB, is what changes the image


def test_seventeen_lines_are_refused_by_name(gpu_device):
    case = _case(53, 37, 2, _random_atlas(), seed=3, L=17)
    fr = torch.from_numpy(case["frames"]).to(gpu_device)
    with pytest.raises(_lib.PoseRiskHipError, match=r"\(status -1\): pr_compose_video: L = 17 lines outside 0\.\.16$") as e:
        video.compose(fr, case["src_idx"], case["box"], case["lines"], case["text"], case["atlas"], 31, 40, 23)
    assert "pr_compose_people" not in str(e.value)


def test_panel_free_and_index_free_forms(gpu_device):
    """No lines (an empty panel), no box, no src_idx (canvas n shows frame n), panel_w = 0."""
    H, W = 37, 53
    frames = _frames(H, W, 1)
    fr = torch.from_numpy(frames).to(gpu_device)
    out = video.compose(fr, dst_h=29, dst_w=41, panel_w=6).cpu().numpy()
    for n in range(N_FRAMES):
        np.testing.assert_array_equal(out[n, :, :41], vr.area_resample(frames[n], 29, 41))
    assert not out[:, :, 41:].any()
    out = video.compose(fr, dst_h=90, dst_w=117, panel_w=0).cpu().numpy()
    np.testing.assert_array_equal(out[2], vr.area_resample(frames[2], 90, 117))
    with pytest.raises(_lib.PoseRiskHipError):
        video.compose(torch.from_numpy(frames))                   # no CPU fallback
    with pytest.raises(ValueError):
        video.compose(fr, box=np.zeros((2, 4), np.int32))


def test_canvas_is_independent_of_its_batch(gpu_device):
    case = _case(450, 800, 64, video.font_atlas(), seed=21)
    case["frames"] = torch.from_numpy(case["frames"]).to(gpu_device)
    whole = _run(case, gpu_device).cpu().numpy()
    again = _run(case, gpu_device).cpu().numpy()
    assert whole.tobytes() == again.tobytes()
    for n in (0, 3, 13, 38, 63):
        alone = _run(case, gpu_device, sel=slice(n, n + 1)).cpu().numpy()
        assert alone[0].tobytes() == whole[n].tobytes(), n
    parts = np.concatenate([_run(case, gpu_device, sel=slice(k, k + 16)).cpu().numpy() for k in range(0, 64, 16)])
    assert parts.tobytes() == whole.tobytes()


def test_compose_is_capturable(gpu_device):
    """One capture on a single stream, replayed once, gives the eager bits."""
    case = _case(450, 800, 7, video.font_atlas(), seed=31)
    dev = gpu_device
    t = {k: torch.from_numpy(np.ascontiguousarray(case[k])).to(dev) for k in ("frames", "src_idx", "box", "lines", "text")}
    cov = torch.from_numpy(np.array(case["atlas"].cov)).to(dev)
    atlas = (cov, case["atlas"].adv, case["atlas"].ascent)
    shape = (7, case["dst_h"], case["dst_w"] + case["panel_w"], 3)
    call = lambda out: video.compose(t["frames"], t["src_idx"], t["box"], t["lines"], t["text"], atlas, case["dst_h"], case["dst_w"],
                                     case["panel_w"], box_rgb=BOX_RGB, out=out)
    eager = call(torch.empty(shape, dtype=torch.uint8, device=dev)).clone()
    static = torch.zeros(shape, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call(static)
    static.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(static, eager)
    assert eager.cpu().numpy()[1].tobytes() == _reference(case, [1])[0][1].tobytes()


# ---- end to end: Predictor.__call__ with the gpu_video knob -----------------------------------------------------------
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
    args = types.SimpleNamespace(gpu="0", type="REBA,RULA", debug=False, debug_joints="", debug_frame=-1, **knobs)
    return base.Predictor(args, spin_model=model, smpl_model=smpl, batch_size=4)


def _clip(tmp_path):
    """The synthetic clip of tests/test_render_gpu.py: 9 frames of 320 x 240, a track over frames 1-6 and 8."""
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


def _no_cv2(monkeypatch):
    """Make `import cv2` raise ImportError for this test, so that the writers take their PNG branch (whose bytes can be compared)
    whether or not OpenCV is installed."""
    monkeypatch.setitem(sys.modules, "cv2", None)


def _draw(pred, out, title, n_frames):
    _, scores, logs, _ = out[title.lower()]
    items = (pred.reba if title == "REBA" else pred.rula).eval_items
    return video.draw_list(title, n_frames, out['bboxes'], (0, out['frames'], n_frames), scores, items, logs, 540)


def test_predictor_call_writes_the_gpu_video(gpu_device, tmp_path, capsys, monkeypatch):
    from PIL import Image
    _no_cv2(monkeypatch)
    frames, src = _clip(tmp_path)
    pred = _predictor(gpu_device, gpu_video=True)
    assert pred.gpu_video and not pred.render_mesh
    out = pred(src, "", str(tmp_path / "out"))
    assert "skipped" not in capsys.readouterr().out
    fr_dev = torch.from_numpy(frames).to(gpu_device)
    for title in ("REBA", "RULA"):
        pngs = sorted((tmp_path / "out" / f"{title}_video").iterdir())
        assert [p.name for p in pngs] == ['{0:09d}.png'.format(i) for i in range(9)]        # every frame of the video
        draw = _draw(pred, out, title, 9)
        lines, codes = video.pack_lines(draw.text)
        want = video.compose(fr_dev, None, draw.box, lines, codes).cpu().numpy()
        assert want.shape == (9, 540, 1000, 3)
        for i, p in enumerate(pngs):
            np.testing.assert_array_equal(np.asarray(Image.open(p)), want[i], err_msg=f"{title} frame {i}")
        # ... which is the contract's canvas: a track frame and one without a target
        a = video.font_atlas()
        ref, _ = vr.compose(frames, None, draw.box, lines, codes, np.asarray(a.cov), a.adv, a.ascent, 540, 720, 280, video.GREEN,
                            canvases=[0, 2])
        for i in (0, 2):
            assert want[i].tobytes() == ref[i].tobytes()
        assert want[2, :, 720:].any() and (want[2, :, :720] == (0, 255, 0)).all(axis=2).any()


def test_predictor_gpu_video_over_the_mesh(gpu_device, tmp_path, monkeypatch):
    """gpu_video with render_mesh: a track frame's image region is the mesh-overlaid frame with the box over it."""
    from PIL import Image
    _no_cv2(monkeypatch)
    frames, src = _clip(tmp_path)
    pred = _predictor(gpu_device, gpu_video=True, render_mesh=True)
    out = pred(src, "", str(tmp_path / "out"))
    for title in ("REBA", "RULA"):
        draw = _draw(pred, out, title, 9)
        got = {int(f): img.cpu().numpy() for fs, imgs in pred.render_overlay(out, frames, title) for f, img in zip(fs, imgs)}
        assert sorted(got) == out['frames'].tolist()
        for f in (1, 4, 8, 0, 7):                                  # track frames, and two without a target (plain)
            png = np.asarray(Image.open(tmp_path / "out" / f"{title}_video" / '{0:09d}.png'.format(f)))
            src_img = got.get(f, frames[f])
            want = vr.area_resample(vr.draw_box(src_img, draw.box[f], video.GREEN), 540, 720)
            np.testing.assert_array_equal(png[:, :720], want, err_msg=f"{title} frame {f}")
        assert (got[4] != frames[4]).any()                         # the mesh is there
        assert (tmp_path / "out" / f"{title}_mesh").is_dir()       # and its own output is still written


def test_predictor_knob_off_changes_nothing(gpu_device, tmp_path, capsys, monkeypatch):
    _no_cv2(monkeypatch)
    frames, src = _clip(tmp_path)
    pred = _predictor(gpu_device)
    assert pred.gpu_video is False
    pred(src, "", str(tmp_path / "off"))
    printed = capsys.readouterr().out
    names = [p.name for p in (tmp_path / "off").iterdir()]
    assert not any("_video" in n for n in names), names
    assert "the annotated mp4 is skipped" in printed
    assert "reba_result.txt" in names and "REBA_score.png" in names
