"""Annotated score video: every video frame resized to 720 px wide with the target's box, beside a 280 px panel with the frame
number, the REBA / RULA score and the per-part scores -- the reference's `<TITLE>_video.mp4` (lib/core/base.py:284-327,
vis_utils.py:278-294) composed on the GPU (include/poserisk_hip.h, pr_compose_video; the kernel is csrc/compose.hip).

`draw_list` is the host half: the strings, origins, sizes, colours and box corners `reports.write_annotated_video` hands to
OpenCV, per video frame.  `font_atlas` is the panel's font: a monospace coverage atlas in three sizes.  `compose` is the torch
wrapper of the kernel, `annotated_frames` chains them batch by batch.  The Predictor's `write_gpu_video`
(dropin/core/outputs.py) writes what it yields.

The people video (`<TITLE>_people`, the persons knob; no counterpart in the reference) is the second half of this file:
`people_draw_list`, `compose_people` (pr_compose_people: the same kernel in csrc/compose.hip, of which pr_compose_video is the
case of one box and no tags), `people_frames`, written by the Predictor's `write_people_video`."""
import collections
import os

import numpy as np
import torch

from . import _lib

RESIZE_W, PANEL_W = 720, 280          # base.py:287, 290
TEXT_X = RESIZE_W + 15                # base.py:296 ff.: every line starts at x = 735
MAX_LINES, LINE_INTS = 16, 5          # PR_VIDEO_MAX_LINES, PR_VIDEO_LINE_INTS
GREEN, WHITE = (0, 255, 0), (255, 255, 255)     # the same in RGB and BGR
NO_BOX = (0, 0, -1, -1)
# cv2.putText's fontScale -> size class of the atlas
SIZE_CLASS = {0.5: 0, 0.6: 1, 0.7: 2}
# Pixel sizes standing in for FONT_HERSHEY_SIMPLEX at scales 0.5 / 0.6 / 0.7 (capital height 11 / 13 / 15 px): DejaVu Sans
# Mono's capitals are 0.73 em, its advance 0.60 em -> 9 / 11 / 13 px a character.  The longest lines the reports produce are
# 24 characters in class 0 ("Wrist_twist (L,R): 10,10" -> 216 px), 19 in class 1 ("Not detected target" -> 209 px) and 14 in
# class 2 ("REBA Score: 15" -> 182 px): all inside the 265 px between x = 735 and the canvas edge.
FONT_PX = (15, 18, 21)
CELL_H, CELL_W = 28, 16
HINTING = 8                           # matplotlib's own horizontal oversampling of the hinter

Atlas = collections.namedtuple("Atlas", "cov adv ascent")     # u8[S,96,CELL_H,CELL_W], S ints, S ints
DrawList = collections.namedtuple("DrawList", "text box")     # per frame [(string, (x, baseline y), class, colour)], int32[F,4]

_atlas = None
_atlas_dev = {}


def font_atlas():
    """The panel's font, rasterised once per process: DejaVu Sans Mono (the file matplotlib ships) through matplotlib.ft2font
    at FONT_PX, as 8-bit coverage.  Atlas(cov u8[3,96,CELL_H,CELL_W] for codes 32..127, adv (px per character), ascent (rows
    from a cell's top to the baseline)).  A glyph sits in its cell at its own bearing."""
    global _atlas
    if _atlas is not None:
        return _atlas
    import matplotlib
    from matplotlib import ft2font
    path = os.path.join(matplotlib.get_data_path(), "fonts", "ttf", "DejaVuSansMono.ttf")
    font = ft2font.FT2Font(path, hinting_factor=HINTING)
    cov = np.zeros((len(FONT_PX), 96, CELL_H, CELL_W), np.uint8)
    adv, ascent = [], []
    import warnings
    for s, px in enumerate(FONT_PX):
        font.set_size(px, 72)                                   # points at 72 dpi = pixels
        asc = -(-font.ascender * px // font.units_per_EM)       # ceil
        adv.append(int(round(font.load_char(ord("M")).linearHoriAdvance / 65536.0)))
        ascent.append(int(asc))
        for code in range(33, 128):
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")                  # code 127 has no glyph: the font's "missing" box stands in
                font.set_text(chr(code), 0.0)
                font.draw_glyphs_to_bitmap(antialiased=True)
                img = np.asarray(font.get_image())
                # the bitmap spans the glyph's box (26.6 fixed point, y up from the baseline, x in 1/8 px steps of the
                # hinter) with one spare row above it
                xmin, _, _, ymax = font.load_char(code).bbox
            if img.size == 0:
                continue
            x0, y0 = xmin // (64 * HINTING), asc - ymax // 64 - 1
            h, w = img.shape
            ys, xs = max(0, -y0), max(0, -x0)                     # clip to the cell
            ye, xe = min(h, CELL_H - y0), min(w, CELL_W - x0)
            if ye > ys and xe > xs:
                cov[s, code - 32, y0 + ys:y0 + ye, x0 + xs:x0 + xe] = img[ys:ye, xs:xe]
    cov.setflags(write=False)
    _atlas = Atlas(cov, tuple(adv), tuple(ascent))
    return _atlas


def box_corners(box):
    """(cx, cy, w, h) -> (x_min, y_min, x_max, y_max) with the reference's integer arithmetic (vis_utils.py:280-283,
    reports.draw_track_box)."""
    return (int(box[0]) - int(box[2]) // 2, int(box[1]) - int(box[3]) // 2,
            int(box[0]) + int(box[2]) // 2, int(box[1]) + int(box[3]) // 2)


def draw_list(title, n_frames, bboxes, timestamp, scores, joint_names, logs, canvas_h):
    """What reports.write_annotated_video draws, per video frame, without drawing it: DrawList(text, box).  text[i] lists
    frame i's putText calls in order as (string, (x, baseline y), size class, colour); box[i] is the track box's corners or
    NO_BOX.  Track frames show the numbers of track index `idx // 2 * 2` (the reference's quirk, Q21), the others
    "Not detected target"."""
    track_frames = np.asarray(timestamp[1])
    text, box = [], np.tile(np.array(NO_BOX, np.int32), (n_frames, 1))
    for i in range(n_frames):
        lines = [("frame: " + str(i), (TEXT_X, canvas_h - 14), 0, WHITE)]
        hit = np.where(track_frames == i)[0]
        if hit.size:
            idx = int(hit[0]) // 2 * 2
            box[i] = box_corners(bboxes[idx])
            lines.append((title + " Score: " + str(scores[idx]), (TEXT_X, 35), 2, GREEN))
            lines.append(("- Score per Joints ", (TEXT_X, 122), 1, WHITE))
            for j, joint in enumerate(joint_names):
                lines.append((joint + ": " + str(logs[idx][j]), (TEXT_X, 153 + 24 * j), 0, WHITE))
        else:
            lines.append(("Not detected target", (TEXT_X, canvas_h - 65), 1, WHITE))
        text.append(lines)
    return DrawList(text, box)


def pack_lines(text, L=None, C=None, max_lines=MAX_LINES):
    """text (DrawList.text, or any per-canvas lists of (string, (x, y), class, colour)) -> lines int32[N,L,5], codes u8[N,L,C]
    as pr_compose_video takes them (max_lines=PEOPLE_MAX_LINES: as pr_compose_people does).  Characters outside Latin-1 become '?'."""
    n = len(text)
    L = max([len(t) for t in text] + [1]) if L is None else L
    C = max([len(s[0]) for t in text for s in t] + [1]) if C is None else C
    if L > max_lines:
        raise ValueError(f"{L} lines per canvas: {'pr_compose_video' if max_lines == MAX_LINES else 'pr_compose_people'} takes at most {max_lines}")
    lines = np.zeros((n, L, LINE_INTS), np.int32)
    codes = np.zeros((n, L, C), np.uint8)
    for i, t in enumerate(text):
        if len(t) > L:
            raise ValueError(f"canvas {i} has {len(t)} lines, L = {L}")
        for l, (string, (x, y), cls, col) in enumerate(t):
            raw = string.encode("latin-1", "replace")[:C]
            lines[i, l] = (x, y, cls, len(raw), int(col[0]) | int(col[1]) << 8 | int(col[2]) << 16)
            codes[i, l, :len(raw)] = np.frombuffer(raw, np.uint8)
    return lines, codes


def canvas_size(H, W):
    """(dst_h, dst_w, panel_w) of the reference's canvas for H x W frames (base.py:287-290)."""
    return int(H * RESIZE_W / W), RESIZE_W, PANEL_W


def _dev(x, dtype, dev, shape, what):
    t = torch.as_tensor(x).to(device=dev, dtype=dtype).contiguous()
    if t.dim() != len(shape) or any(s is not None and t.shape[i] != s for i, s in enumerate(shape)):
        raise ValueError(f"{what} must have shape {shape}, got {tuple(t.shape)}")
    return t


def _canvas_args(who, frames, src_idx, lines, text, atlas, dst_h, dst_w, panel_w, out, return_status):
    """The argument checks and uploads compose and compose_people share -> (frames, idx, ln, tx, cov, out, st, N, dst_h, L, C, S,
    CH, CW, adv, ascent)."""
    if not (isinstance(frames, torch.Tensor) and frames.device.type == "cuda"):
        raise _lib.PoseRiskHipError(f"{who}: frames must be a CUDA tensor (no CPU fallback)")
    if frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[3] != 3:
        raise ValueError("frames must be uint8 [n_frames,H,W,3]")
    dev = frames.device
    frames = frames.contiguous()
    n_frames, H, W, _ = frames.shape
    if dst_h is None:
        dst_h = int(H * dst_w / W)
    if src_idx is not None:
        idx = _dev(src_idx, torch.int32, dev, (None,), "src_idx")
        N = idx.shape[0]
    else:
        idx, N = None, n_frames
    if (lines is None) != (text is None):
        raise ValueError("lines and text come together (pack_lines)")
    ln = tx = cov = None
    L = C = S = CH = CW = 0
    adv = ascent = ()
    if lines is not None:
        ln = _dev(lines, torch.int32, dev, (N, None, LINE_INTS), "lines")
        L = ln.shape[1]
        tx = _dev(text, torch.uint8, dev, (N, L, None), "text")
        C = tx.shape[2]
        if atlas is None:
            atlas = font_atlas()
            key = (dev.type, dev.index if dev.index is not None else torch.cuda.current_device())
            if key not in _atlas_dev:
                _atlas_dev[key] = torch.from_numpy(np.array(atlas.cov)).to(dev)       # a writable copy, uploaded once
            cov = _atlas_dev[key]
        else:
            cov = _dev(atlas[0], torch.uint8, dev, (None, 96, None, None), "atlas coverage")
        adv, ascent = [int(v) for v in atlas[1]], [int(v) for v in atlas[2]]
        S, CH, CW = cov.shape[0], cov.shape[2], cov.shape[3]
        if len(adv) != S or len(ascent) != S or S > 4:
            raise ValueError(f"atlas with {S} size classes (at most 4) needs {S} advances and ascents, got {len(adv)}, {len(ascent)}")
    shape = (N, dst_h, dst_w + panel_w, 3)
    if out is None:
        out = torch.empty(shape, dtype=torch.uint8, device=dev)
    elif tuple(out.shape) != shape or out.dtype != torch.uint8 or not out.is_contiguous() or out.device != dev:
        raise ValueError(f"out must be a contiguous uint8 {list(shape)} tensor on the frames' device")
    st = torch.empty((N,), dtype=torch.int32, device=dev) if return_status else None
    return frames, idx, ln, tx, cov, out, st, N, dst_h, L, C, S, CH, CW, adv, ascent


def compose(frames, src_idx=None, box=None, lines=None, text=None, atlas=None, dst_h=None, dst_w=RESIZE_W, panel_w=PANEL_W,
            box_rgb=GREEN, out=None, return_status=False):
    """Compose N canvases on the GPU.

    frames u8[n_frames,H,W,3] CUDA; src_idx int[N] or None (canvas n shows frame n, N = n_frames); box int[N,4] (x_min, y_min,
    x_max, y_max; x_max < x_min: none) or None; lines int[N,L,5] + text u8[N,L,C] (pack_lines) or None (an empty panel);
    atlas: Atlas or (cov u8[S,96,CH,CW], adv, ascent), default font_atlas(); dst_h default int(H * dst_w / W); box_rgb in the
    frames' channel order.  Returns out u8[N,dst_h,dst_w+panel_w,3], and status int32[N] when asked for.

    Arguments given as numpy arrays (or on another device) are uploaded on every call with a blocking copy -- a caller-supplied
    numpy atlas included; only the default atlas is cached per device.  Pass CUDA tensors of the right dtype (int32 src_idx, box
    and lines, uint8 text and atlas coverage) and `out` to make the call free of copies and allocation, which is what capturing
    it into a graph needs."""
    frames, idx, ln, tx, cov, out, st, N, dst_h, L, C, S, CH, CW, adv, ascent = _canvas_args(
        "compose", frames, src_idx, lines, text, atlas, dst_h, dst_w, panel_w, out, return_status)
    dev, (n_frames, H, W, _) = frames.device, frames.shape
    bx = _dev(box, torch.int32, dev, (N, 4), "box") if box is not None else None
    ptr = lambda t: t.data_ptr() if t is not None else None
    pad = lambda v: (_lib.C.c_int * 4)(*(list(v) + [0] * (4 - len(v))))
    args = _lib.ComposeArgs(frames.data_ptr(), ptr(idx), ptr(bx), ptr(ln), ptr(tx), ptr(cov), out.data_ptr(), ptr(st),
                            N, n_frames, H, W, dst_h, dst_w, panel_w, L, C, S, CH, CW, pad(adv), pad(ascent),
                            (_lib.C.c_uint8 * 4)(int(box_rgb[0]), int(box_rgb[1]), int(box_rgb[2]), 0))
    _lib.check(_lib.load().pr_compose_video(args, torch.cuda.current_stream(dev).cuda_stream), "pr_compose_video")
    return (out, st) if return_status else out


def annotated_frames(frames, draw, batch_size=64, atlas=None, overlay=None):
    """Yield the canvases of the whole video in order, `batch_size` video frames at a time, as CUDA u8[b,dst_h,1000,3] in the
    frames' channel order.  frames u8[F,H,W,3] CUDA; draw = draw_list(..., canvas_h=canvas_size(H, W)[0]).  `overlay(lo, hi)`,
    when given, returns (frame numbers int[m], images u8[m,H,W,3] CUDA) for the frames in [lo, hi) that have a drawn-over
    version (Predictor.render_overlay's mesh): those replace the plain frames, under the box."""
    if not (isinstance(frames, torch.Tensor) and frames.device.type == "cuda"):
        raise _lib.PoseRiskHipError("annotated_frames: frames must be a CUDA tensor (no CPU fallback)")
    F, H, W = int(frames.shape[0]), int(frames.shape[1]), int(frames.shape[2])
    if len(draw.text) != F:
        raise ValueError(f"the draw list has {len(draw.text)} frames, the video {F}")
    dst_h, dst_w, panel_w = canvas_size(H, W)
    L = max(len(t) for t in draw.text) if F else 1
    C = max(len(s[0]) for t in draw.text for s in t) if F else 1
    for lo in range(0, F, batch_size):
        hi = min(lo + batch_size, F)
        lines, codes = pack_lines(draw.text[lo:hi], L, C)
        src, idx = frames, np.arange(lo, hi, dtype=np.int32)
        if overlay is not None:
            numbers, images = overlay(lo, hi)
            if len(numbers):
                src = frames[lo:hi].clone()
                src[torch.as_tensor(np.asarray(numbers) - lo, device=src.device, dtype=torch.long)] = images
                idx = None
        yield compose(src, idx, draw.box[lo:hi], lines, codes, atlas, dst_h, dst_w, panel_w)


# ---- the people video (pr_compose_people): every tracked person's box and tag on the frame, a people panel beside it ----------
PEOPLE_MAX_BOXES, PEOPLE_MAX_LINES = 16, 32     # PR_PEOPLE_MAX_BOXES, PR_PEOPLE_MAX_LINES
PEOPLE_PANEL_ROWS = 14                          # people listed in the panel at most
# Box, tag and panel-line colour by action level 1 .. 5 (REBA has five levels, RULA four), RGB: render.LEVEL_RGB's four, then a
# purple for REBA's "very high risk"
PEOPLE_LEVEL_RGB = ((40, 200, 60), (250, 220, 40), (250, 140, 20), (230, 30, 30), (170, 40, 200))
TAG_GAP = 3                                     # px between a tag's baseline and the box's top edge
TAG_H = FONT_PX[0]                              # rows a class-0 tag needs above its baseline to stay on the canvas
PANEL_CHARS = (PANEL_W - 15) // 9               # class-0 characters between TEXT_X and the canvas edge (FONT_PX's comment: 9 px each)
NO_LINE = ("", (0, 0), 0, (0, 0, 0))            # a slot that draws nothing (length 0)

PeopleDraw = collections.namedtuple("PeopleDraw", "tags panel box box_rgb")     # per frame lists of lines; int32[F,K,4], u8[F,K,4]


def people_draw_list(title, n_frames, people, canvas_h, dst_w, H, W, bgr=False):
    """What the people video shows, per video frame, without drawing it: PeopleDraw(tags, panel, box, box_rgb).

    people: one dict per person in tracks.people_tracks order, with 'id', 'frames' int[n], 'bboxes' f32[n,4] (cx, cy, w, h),
    'scores' int[n], 'levels' int[n] (the action level of each frame's score, 1 .. 5; anything else counts as 1) and 'names'
    (the action name of each frame's score).  A frame shows each person's OWN score of that frame: the `idx // 2 * 2` indexing
    of draw_list is the single-target video's quirk (the reference's, Q21) and is not carried over.

    Frame i draws the people whose track has frame i (the first row that names it), in the order given; more than
    PEOPLE_MAX_BOXES of them: the 16 with the largest boxes (w * h of that frame, ties to the earlier person), still in the
    order given.  Per person: box[i][k] = box_corners of the frame's box, box_rgb[i][k] = PEOPLE_LEVEL_RGB[level - 1] (swapped
    with bgr), and the tag `#<id> <score>` in that colour at size class 0, its origin the box's top-left corner mapped to
    the canvas, (floor(x_min dst_w / W), floor(y_min canvas_h / H)), its baseline TAG_GAP px above that corner -- or, where fewer
    than TAG_H rows would be left above the baseline, TAG_GAP + TAG_H px below it.  The panel: `<TITLE> people: k` (k: the
    people visible in the frame, all of them) in draw_list's score colour, then `#<id>  <score>  <action name>` per drawn
    person in their colour, PEOPLE_PANEL_ROWS of them at most, cut to PANEL_CHARS characters, then draw_list's `frame: i`.
    K = the most people drawn in one frame (at least 1); unused slots hold NO_BOX."""
    text_x = dst_w + 15
    where = [{int(f): r for r, f in reversed(list(enumerate(np.asarray(p['frames']).tolist())))} for p in people]
    visible = [[(q, where[q][i]) for q in range(len(people)) if i in where[q]] for i in range(n_frames)]
    K = max([min(len(v), PEOPLE_MAX_BOXES) for v in visible] + [1])
    box = np.tile(np.array(NO_BOX, np.int32), (n_frames, K, 1))
    box_rgb = np.zeros((n_frames, K, 4), np.uint8)
    tags, panel = [], []
    for i, vis in enumerate(visible):
        shown = vis
        if len(vis) > PEOPLE_MAX_BOXES:
            area = [float(people[q]['bboxes'][r][2]) * float(people[q]['bboxes'][r][3]) for q, r in vis]
            keep = sorted(sorted(range(len(vis)), key=lambda j: (-area[j], j))[:PEOPLE_MAX_BOXES])
            shown = [vis[j] for j in keep]
        t = []
        lines = [(f"{title} people: {len(vis)}", (text_x, 35), 2, GREEN)]
        for k, (q, r) in enumerate(shown):
            p = people[q]
            level = int(p['levels'][r]) if p['levels'][r] is not None else 1
            rgb = PEOPLE_LEVEL_RGB[level - 1 if 1 <= level <= len(PEOPLE_LEVEL_RGB) else 0]
            rgb = rgb[::-1] if bgr else rgb
            corners = box_corners(p['bboxes'][r])
            box[i, k], box_rgb[i, k, :3] = corners, rgb
            x, y = corners[0] * dst_w // W, corners[1] * canvas_h // H
            yb = y - TAG_GAP if y - TAG_GAP - TAG_H >= 0 else y + TAG_GAP + TAG_H
            t.append((f"#{p['id']} {p['scores'][r]}", (x, yb), 0, rgb))
            if k < PEOPLE_PANEL_ROWS:
                lines.append((f"#{p['id']}  {p['scores'][r]}  {p['names'][r]}"[:PANEL_CHARS], (text_x, 70 + 24 * k), 0, rgb))
        lines.append(("frame: " + str(i), (text_x, canvas_h - 14), 0, WHITE))
        tags.append(t)
        panel.append(lines)
    return PeopleDraw(tags, panel, box, box_rgb)


def compose_people(frames, src_idx=None, box=None, box_rgb=None, lines=None, text=None, L_img=0, atlas=None, dst_h=None,
                   dst_w=RESIZE_W, panel_w=PANEL_W, out=None, return_status=False):
    """Compose N people canvases on the GPU (pr_compose_people; the contract is section r3 of include/poserisk_hip.h).

    As `compose`, with box int[N,K,4] and box_rgb u8[N,K,4] (a colour per slot, in the frames' channel order; [3] unused) in
    place of one box and one colour, up to PEOPLE_MAX_LINES lines, and L_img: lines [0, L_img) are tags, drawn over the image
    region; the others are panel lines.  Returns out u8[N,dst_h,dst_w+panel_w,3], and status int32[N] when asked for."""
    frames, idx, ln, tx, cov, out, st, N, dst_h, L, C, S, CH, CW, adv, ascent = _canvas_args(
        "compose_people", frames, src_idx, lines, text, atlas, dst_h, dst_w, panel_w, out, return_status)
    dev, (n_frames, H, W, _) = frames.device, frames.shape
    if (box is None) != (box_rgb is None):
        raise ValueError("box and box_rgb come together")
    bx = rgb = None
    K = 1
    if box is not None:
        bx = _dev(box, torch.int32, dev, (N, None, 4), "box")
        K = bx.shape[1]
        rgb = _dev(box_rgb, torch.uint8, dev, (N, K, 4), "box_rgb")
    ptr = lambda t: t.data_ptr() if t is not None else None
    pad = lambda v: (_lib.C.c_int * 4)(*(list(v) + [0] * (4 - len(v))))
    args = _lib.ComposePeopleArgs(frames.data_ptr(), ptr(idx), ptr(bx), ptr(rgb), ptr(ln), ptr(tx), ptr(cov), out.data_ptr(), ptr(st),
                                  N, n_frames, H, W, dst_h, dst_w, panel_w, K, L, int(L_img), C, S, CH, CW, pad(adv), pad(ascent))
    _lib.check(_lib.load().pr_compose_people(args, torch.cuda.current_stream(dev).cuda_stream), "pr_compose_people")
    return (out, st) if return_status else out


def pack_people(draw, lo, hi, n_tags=None, L=None, C=None):
    """Frames [lo, hi) of a PeopleDraw -> (lines int32[n,L,5], codes u8[n,L,C], L_img) as pr_compose_people takes them: every
    frame's tags padded with NO_LINE to n_tags slots (default: the box slots), then its panel lines."""
    n_tags = draw.box.shape[1] if n_tags is None else n_tags
    both = [list(t) + [NO_LINE] * (n_tags - len(t)) + list(p) for t, p in zip(draw.tags[lo:hi], draw.panel[lo:hi])]
    lines, codes = pack_lines(both, L, C, max_lines=PEOPLE_MAX_LINES)
    return lines, codes, n_tags


def people_frames(frames, draw, batch_size=64, atlas=None, overlay=None):
    """Yield the people canvases of the whole video in order, `batch_size` video frames at a time, as CUDA u8[b,dst_h,1000,3]
    in the frames' channel order.  frames u8[F,H,W,3] CUDA; draw = people_draw_list(..., canvas_size(H, W)[0], RESIZE_W, H, W).
    `overlay(lo, hi)`, as annotated_frames': (frame numbers int[m], images u8[m,H,W,3] CUDA) for the frames in [lo, hi) that
    have a drawn-over version (Predictor.render_people's meshes): those replace the plain frames, under the boxes and tags."""
    if not (isinstance(frames, torch.Tensor) and frames.device.type == "cuda"):
        raise _lib.PoseRiskHipError("people_frames: frames must be a CUDA tensor (no CPU fallback)")
    F, H, W = int(frames.shape[0]), int(frames.shape[1]), int(frames.shape[2])
    if len(draw.panel) != F:
        raise ValueError(f"the draw list has {len(draw.panel)} frames, the video {F}")
    dst_h, dst_w, panel_w = canvas_size(H, W)
    n_tags = draw.box.shape[1]
    L = n_tags + (max(len(p) for p in draw.panel) if F else 1)
    C = max([len(s[0]) for group in (draw.tags, draw.panel) for t in group for s in t] + [1])
    for lo in range(0, F, batch_size):
        hi = min(lo + batch_size, F)
        lines, codes, L_img = pack_people(draw, lo, hi, n_tags, L, C)
        src, idx = frames, np.arange(lo, hi, dtype=np.int32)
        if overlay is not None:
            numbers, images = overlay(lo, hi)
            if len(numbers):
                src = frames[lo:hi].clone()
                src[torch.as_tensor(np.asarray(numbers) - lo, device=src.device, dtype=torch.long)] = images
                idx = None
        yield compose_people(src, idx, draw.box[lo:hi], draw.box_rgb[lo:hi], lines, codes, L_img, atlas, dst_h, dst_w, panel_w)
