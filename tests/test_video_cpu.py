"""CPU-only: the host half of the annotated score video (poserisk_release_amd/video.py), the numpy restatement of the compose
contract (tests/video_ref.py) against an independent float64 formulation, and pr_compose_video's argument checks."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest

import video_ref as vr
from conftest import REPO
from poserisk_release_amd import _lib, reports, video


# ---- area resample ---------------------------------------------------------------------------------------------------
def _summed_area(img, dst_h, dst_w):
    """The box filter from a float64 summed-area table: the image is piecewise constant, so its integral over
    [0, y) x [0, x) is the table interpolated linearly along both axes; a destination cell's mean is the integral over its
    footprint [i H / dst_h, (i+1) H / dst_h) x [l W / dst_w, (l+1) W / dst_w) divided by the footprint's area."""
    H, W = img.shape[:2]
    P = np.zeros((H + 1, W + 1, 3), np.float64)
    P[1:, 1:] = np.cumsum(np.cumsum(img.astype(np.float64), axis=0), axis=1)

    def lerp(T, t, axis, n):
        a = np.minimum(np.floor(t), n - 1).astype(np.int64)
        f = (t - a).reshape([-1 if k == axis else 1 for k in range(3)])
        return np.take(T, a, axis=axis) * (1.0 - f) + np.take(T, a + 1, axis=axis) * f

    ye = np.arange(dst_h + 1, dtype=np.float64) * H / dst_h
    xe = np.arange(dst_w + 1, dtype=np.float64) * W / dst_w
    I = lerp(lerp(P, ye, 0, H), xe, 1, W)
    return (I[1:, 1:] - I[:-1, 1:] - I[1:, :-1] + I[:-1, :-1]) / ((H / dst_h) * (W / dst_w))


@pytest.mark.parametrize("H,W", [(450, 800), (1080, 1920), (449, 799), (480, 640), (37, 53)])
def test_area_resample_is_the_box_filter(H, W):
    img = np.random.default_rng(H + W).integers(0, 256, (H, W, 3), dtype=np.uint8)
    dst_h, dst_w, _ = video.canvas_size(H, W)
    got = vr.area_resample(img, dst_h, dst_w)
    assert got.shape == (dst_h, dst_w, 3) and got.dtype == np.uint8
    err = float(np.abs(got.astype(np.float64) - _summed_area(img, dst_h, dst_w)).max())
    print(f"[video] {H}x{W} -> {dst_h}x{dst_w}: max |integer - float64 summed-area| = 0.5 + {err - 0.5:.3e}")
    # rounding alone gives 0.5; 1e-4 covers float64 error on prefix sums up to 2^33
    assert err <= 0.5 + 1e-4


def test_area_resample_special_cases():
    rng = np.random.default_rng(0)
    img = rng.integers(0, 256, (48, 60, 3), dtype=np.uint8)
    # an integer ratio is the block mean, rounded half to even
    mean = img.reshape(12, 4, 20, 3, 3).astype(np.int64).sum(axis=(1, 3))
    q, r = np.divmod(mean, 12)
    want = q + ((2 * r > 12) | ((2 * r == 12) & (q % 2 == 1)))
    np.testing.assert_array_equal(vr.area_resample(img, 12, 20), want.astype(np.uint8))
    # the same size is the identity -- a 720-wide input at the reference's canvas size
    wide = rng.integers(0, 256, (30, 720, 3), dtype=np.uint8)
    assert video.canvas_size(30, 720) == (30, 720, 280)
    np.testing.assert_array_equal(vr.area_resample(wide, 30, 720), wide)
    # a constant image stays constant, up and down, at awkward ratios
    for v in (0, 1, 127, 255):
        flat = np.full((37, 53, 3), v, np.uint8)
        for dh, dw in ((29, 41), (90, 117), (1, 1)):
            assert (vr.area_resample(flat, dh, dw) == v).all()
    # the weights: every row of the overlap matrix sums to the source length
    for n_src, n_dst in ((800, 720), (1920, 720), (53, 720), (7, 7)):
        o = vr.overlaps(n_src, n_dst)
        assert (o.sum(axis=1) == n_src).all() and (o.sum(axis=0) == n_dst).all()
    assert int((vr.overlaps(800, 720) > 0).sum(axis=1).max()) == 2 and int((vr.overlaps(1920, 720) > 0).sum(axis=1).max()) == 4


def test_box_outline_contract():
    img = np.zeros((20, 30, 3), np.uint8)
    got = vr.draw_box(img, (5, 4, 15, 12), (1, 2, 3))
    on = (got == (1, 2, 3)).all(axis=2)
    assert on[3:14, 4:17].sum() == on.sum()                       # nothing outside [x_min-1, x_max+1] x [y_min-1, y_max+1]
    assert on[3:6, 4:17].all() and on[11:14, 4:17].all() and on[3:14, 4:7].all() and on[3:14, 14:17].all()   # 3 px thick
    assert not on[6:11, 7:14].any()                               # the inside is left alone
    assert (vr.draw_box(img, (0, 0, -1, -1), (9, 9, 9)) == 0).all()       # no box
    assert (vr.draw_box(img, (100, 100, 140, 150), (9, 9, 9)) == 0).all()  # wholly off the frame
    thin = (vr.draw_box(img, (5, 4, 7, 12), (9, 9, 9)) == 9).all(axis=2)  # thinner than 4 px: solid
    assert thin[3:14, 4:9].all() and thin.sum() == 11 * 5
    part = (vr.draw_box(img, (-5, -5, 10, 8), (9, 9, 9)) == 9).all(axis=2)   # partly off: clipped
    assert part[0:10, 9:12].all() and part[7:10, 0:12].all() and not part[0:7, 0:9].any()


# ---- the draw list against the OpenCV writer ------------------------------------------------------------------------
def _recording_cv2(calls):
    cv2 = types.SimpleNamespace(FONT_HERSHEY_SIMPLEX=0, LINE_AA=16, INTER_AREA=3)

    class Writer:
        def __init__(self, path, fourcc, fps, size): calls["open"] = (path, fourcc, fps, size)
        def write(self, frame): calls["frames"].append(frame.shape)
        def release(self): pass
    cv2.VideoWriter = Writer
    cv2.putText = lambda img, text, org, font, scale, color, thick, line: calls["text"].append(
        (len(calls["frames"]), text, org, scale, color))
    cv2.line = lambda img, a, b, color, thick: (calls["lines"].append((len(calls["frames"]), a, b, color, thick)), img)[1]
    cv2.resize = lambda img, wh, interpolation=None: np.zeros((wh[1], wh[0], 3), np.uint8)
    return cv2


def _scheme_inputs(title, n_track, seed):
    from poserisk_release_amd import dropin
    dropin.install()
    from reba import REBA
    from rula import RULA
    items = (REBA if title == "REBA" else RULA)(False).eval_items
    rng = np.random.default_rng(seed)
    logs = np.array([[f"{rng.integers(1, 7)},{rng.integers(1, 7)}" if "(L,R)" in it else str(rng.integers(1, 7)) for it in items]
                     for _ in range(n_track)])
    scores = rng.integers(1, 16, n_track)
    bboxes = np.stack([rng.uniform(40, 200, n_track), rng.uniform(40, 160, n_track), rng.uniform(1, 130, n_track),
                       rng.uniform(1, 170, n_track)], 1).astype(np.float32)
    return items, logs, scores, bboxes


@pytest.mark.parametrize("title", ["REBA", "RULA"])
def test_draw_list_matches_the_opencv_writer(tmp_path, title):
    track = np.array([1, 2, 3, 5, 6, 9, 10])                     # gaps: frames 0, 4, 7, 8, 11 have no target
    n_frames = 12
    items, logs, scores, bboxes = _scheme_inputs(title, len(track), seed=3)
    ts = (0, track, n_frames)
    frames = [np.zeros((240, 320, 3), np.uint8) for _ in range(n_frames)]
    calls = dict(text=[], lines=[], frames=[])
    path = reports.write_annotated_video(str(tmp_path), title, frames, bboxes, ts, 25.0, scores, items, logs,
                                         cv2=_recording_cv2(calls))
    assert path is not None and calls["open"][3] == (1000, 540)
    canvas_h = video.canvas_size(240, 320)[0]
    assert canvas_h == 540
    draw = video.draw_list(title, n_frames, bboxes, ts, scores, items, logs, canvas_h)
    assert len(draw.text) == n_frames and draw.box.shape == (n_frames, 4) and draw.box.dtype == np.int32
    seen_quirk = seen_missing = False
    for i in range(n_frames):
        rec = [(text, tuple(org), video.SIZE_CLASS[scale], tuple(color)) for n, text, org, scale, color in calls["text"] if n == i]
        assert rec == [(s, tuple(o), c, tuple(col)) for s, o, c, col in draw.text[i]], i
        lines = [(a, b) for n, a, b, color, thick in calls["lines"] if n == i]
        x0, y0, x1, y1 = (int(v) for v in draw.box[i])
        if i in track:
            assert lines == [((x0, y0), (x0, y1)), ((x0, y0), (x1, y0)), ((x0, y1), (x1, y1)), ((x1, y0), (x1, y1))], i
            assert all(color == video.GREEN and thick == 2 for n, a, b, color, thick in calls["lines"] if n == i)
            idx = int(np.where(track == i)[0][0])
            if idx % 2:                                           # an odd track index shows its predecessor's numbers
                assert draw.text[i][1][0] == f"{title} Score: {scores[idx - 1]}"
                seen_quirk = True
        else:
            assert lines == [] and x1 < x0
            assert draw.text[i][1][0] == "Not detected target" and draw.text[i][1][1] == (735, canvas_h - 65)
            seen_missing = True
        assert draw.text[i][0] == (f"frame: {i}", (735, canvas_h - 14), 0, video.WHITE)
    assert seen_quirk and seen_missing
    # packed for the kernel: one row per line, Latin-1 codes
    lines, codes = video.pack_lines(draw.text)
    assert lines.shape == (n_frames, 3 + len(items), 5) and codes.dtype == np.uint8 and lines.dtype == np.int32
    s, (x, y), c, col = draw.text[1][1]
    assert lines[1, 1].tolist() == [x, y, c, len(s), col[0] | col[1] << 8 | col[2] << 16]
    assert bytes(codes[1, 1, :len(s)]).decode() == s and lines[0, 2:, 3].tolist() == [0] * (1 + len(items))


# ---- the font ------------------------------------------------------------------------------------------------------------
def test_font_atlas():
    a = video.font_atlas()
    assert a.cov.shape == (3, 96, video.CELL_H, video.CELL_W) and a.cov.dtype == np.uint8
    assert len(a.adv) == 3 and len(a.ascent) == 3 and all(1 <= v <= video.CELL_W for v in a.adv)
    assert list(a.adv) == sorted(a.adv) and a.adv[0] < a.adv[2]                  # three sizes
    for s in range(3):
        seen = a.cov[s, :, :, :a.adv[s]]                          # what the kernel can sample: u < adv
        assert not seen[0].any()                                   # space
        assert all(seen[g].any() for g in range(1, 96)), [g + 32 for g in range(1, 96) if not seen[g].any()]
        assert len({seen[g].tobytes() for g in range(1, 96)}) == 95
        assert int(seen.max()) >= 200                              # real coverage, not a faint smear
    assert video.font_atlas() is a                                 # once per process
    video._atlas = None                                            # ... and rasterised again from scratch: the same bits
    b = video.font_atlas()
    assert b is not a and np.array_equal(a.cov, b.cov) and a.adv == b.adv and a.ascent == b.ascent
    # every line of the two schemes with worst-case logs fits the 265 px between x = 735 and the canvas edge
    for title in ("REBA", "RULA"):
        items, _, _, bboxes = _scheme_inputs(title, 2, seed=1)
        logs = np.array([["10,10" if "(L,R)" in it else "10" for it in items]] * 2)
        draw = video.draw_list(title, 3, bboxes, (0, np.array([0, 1]), 3), np.array([15, 15]), items, logs, 405)
        texts = [t for frame in draw.text for t in frame] + [("frame: 9999999", (735, 391), 0, video.WHITE)]
        assert any(t[0].startswith("Wrist_twist (L,R): ") for t in texts) == (title == "RULA")
        assert any(t[0] == "Not detected target" for t in texts)
        for s, (x, y), c, _ in texts:
            assert x == 735 and len(s) * a.adv[c] <= 265, (s, len(s) * a.adv[c])
            assert y - a.ascent[c] >= 0                            # no line starts above the canvas


# ---- the C ABI -------------------------------------------------------------------------------------------------------------
def test_compose_abi_and_argument_errors():
    hdr = open(os.path.join(REPO, "include", "poserisk_hip.h")).read()
    assert re.search(r"\bint\s+pr_compose_video\s*\(\s*const\s+pr_compose_args\s*\*", hdr)
    assert "pr_compose_video" in _lib.SIGNATURES
    lib = _lib.load()
    assert lib.pr_abi_version() == _lib.ABI_VERSION == 16
    msg = lambda: lib.pr_last_error().decode()
    buf = np.zeros(64, np.uint8)
    p = buf.ctypes.data                                            # never dereferenced: every call below is refused first

    def args(**kw):
        v = dict(frames=p, src_idx=None, box=None, lines=p, text=p, atlas=p, out=p, status=None, N=2, n_frames=2, H=450, W=800,
                 dst_h=405, dst_w=720, panel_w=280, L=3, C=8, S=3, CH=28, CW=16)
        v.update(kw)
        a = _lib.ComposeArgs(**v)
        a.adv[:] = [9, 11, 13, 0]
        a.ascent[:] = [14, 17, 20, 0]
        return a
    call = lambda **kw: lib.pr_compose_video(C.byref(args(**kw)), None)
    assert call(out=None) == -1 and "out" in msg()
    assert call(H=4097) == -1 and "H" in msg() and "4097" in msg()
    assert call(L=17) == -1 and "L = 17" in msg()
    assert call(dst_w=0) == -1 and "dst_w" in msg()
    assert call(frames=None) == -1 and "frames" in msg()
    assert call(atlas=None) == -1 and "atlas" in msg()
    assert call(N=-1) == -1 and "N" in msg()
    assert call(N=3) == -1 and "src_idx" in msg()                  # more canvases than frames without an index
    assert lib.pr_compose_video(None, None) == -1 and "null" in msg()
    assert call(N=0, out=None) == 0                                # an empty batch is legal
