"""Case lists and inputs of the detector's tests (tests/test_detector_gpu.py, tests/test_detector_cpu.py).  A helper module."""
import functools

import numpy as np

from poserisk_release_amd import synth

CONF, NMS = 0.1, 0.4
OBJ_MARGIN, IOU_MARGIN, SCORE_MARGIN = 1e-4, 1e-4, 1e-6        # what the issue sets for "too close to call"

# (id, frame H, frame W, S_h, S_w, bgr, B): wide and tall frames, same size (copy), exactly half (2 x 2 mean), a frame smaller than
# the input (enlarged), bgr, one frame and three
LETTERBOX_CASES = (
    ("wide", 54, 96, 64, 96, False, 3),
    ("tall", 97, 41, 64, 96, False, 1),
    ("same", 64, 96, 64, 96, False, 3),
    ("half", 128, 192, 64, 96, False, 1),
    ("upscale", 23, 31, 64, 96, False, 3),
    ("wide-bgr", 54, 96, 64, 96, True, 1),
    ("odd-into-32x64", 45, 101, 32, 64, True, 3),
)

# the network: input 32 x 64 (the last grid is 1 x 2: every 3 x 3 convolution there is mostly padding) and 64 x 96; B = 1 and 3
NETWORK_SIZES = ((32, 64), (64, 96))
NETWORK_BATCHES = (1, 3)
NETWORK_LAYERS = (0, 1, 4, 36, 61, 74, 79, 85, 86, 97, 98, 82, 94, 106)

POST_SIZE = (128, 160)       # grids 4 x 5, 8 x 10, 16 x 20: 1260 cells a frame, so that more than 1024 candidates fit
DETECT_SIZE = (64, 96)
DETECT_FRAME = (54, 96)      # H, W
DETECT_SEED = 0
# pr_det_detect end to end, (frame H, frame W, bgr) into DETECT_SIZE: the first maps with sx = sy = 1 and ox = 0; (97, 41) has
# ox = 34, sx = 41 / 27, sy = 97 / 64 and kept boxes wholly inside the padding bars; (23, 31) is enlarged (scales below 1, ox = 5);
# (45, 101) has oy = 10 and a scale that is no ratio of small integers, once in RGB and once in BGR.
# Candidates per frame in the float64 reference, none too close to call: 12 11 12 | 14 14 12 | 12 12 11 | 11 13 13 | 13 12 12.
# (97, 41) in BGR order is NOT a case: there frame 1 holds an objectness within OBJ_MARGIN of CONF in the float64 reference, the frame is
# left out whole (13 of 40 candidates) and the cap of 2 % cannot hold whatever the GPU computes.
DETECT_CASES = ((54, 96, False), (97, 41, False), (23, 31, False), (45, 101, False), (45, 101, True))

# pr_det_unmap alone, (frame H, frame W, S_h, S_w): every letterbox case's, the two orientations of a real video, the smallest
# frame, and frames with a side at PR_RESIZE_MAX_SIDE
UNMAP_GEOMETRIES = tuple(dict.fromkeys(c[1:5] for c in LETTERBOX_CASES)) + (
    (1080, 1920, 416, 416), (1920, 1080, 416, 416), (1, 1, 32, 32), (4096, 2304, 416, 416), (300, 4096, 64, 96))
UNMAP_B, UNMAP_MAX_DET, UNMAP_COUNTS = 3, 16, (16, 0, 5)
UNMAP_SENTINEL = np.array([0xC5A5A5A5], np.uint32).view(np.float32)[0]      # finite, negative, and no corner of these tests


@functools.lru_cache(maxsize=1)
def weights():
    w = synth.yolo_weights(seed=11)
    w.setflags(write=False)
    return w


def frames(seed, B, H, W):
    return np.random.default_rng(seed).integers(0, 256, (B, H, W, 3), dtype=np.uint8)


def grids(S_h, S_w):
    return [(S_h // s, S_w // s) for s in (32, 16, 8)]


def crafted_heads(S_h, S_w, seed=3):
    """Three frames of head tensors f32[3,gh,gw,255] made for the post-processing:
      frame 0  about 90 candidates in overlapping clusters (NMS has work), plus cells above the threshold whose best class is not
               0 (left out) and cells whose class 0 ties with another class (kept: the lowest index wins);
      frame 1  nothing above the threshold;
      frame 2  1100 candidates (more than MAX_CAND) with scores on a grid 3e-4 apart and boxes below a pixel: the cut is clean."""
    rng = np.random.default_rng(seed)
    gs = grids(S_h, S_w)
    heads = [np.zeros((3, gh, gw, 3, 85), np.float32) for gh, gw in gs]
    for h in heads:
        h[..., 4] = -8.0                      # objectness 3e-4
        h[..., 5] = 2.0
        h[..., 6:] = -2.0
    cells = [(hd, cy, cx, a) for hd, (gh, gw) in enumerate(gs) for cy in range(gh) for cx in range(gw) for a in range(3)]
    # frame 0
    pick = rng.permutation(len(cells))
    for n, k in enumerate(pick[:130]):
        hd, cy, cx, a = cells[k]
        t = heads[hd][0, cy, cx, a]
        t[0:2] = rng.uniform(-2, 2, 2)
        t[2:4] = rng.uniform(-1.5, 0.5, 2)
        t[4] = rng.uniform(-1, 3)
        t[5] = rng.uniform(0, 3)
        t[6:] = rng.uniform(-3, -0.5, 79)
        if n % 13 == 5:
            t[5 + 1 + int(rng.integers(0, 79))] = t[5] + 1.0        # another class wins: no person
        if n % 13 == 7:
            t[5 + 1 + int(rng.integers(0, 79))] = t[5]              # a tie: class 0 wins
    # frame 2
    pick = rng.permutation(len(cells))[:1100]
    for tc, k in zip(rng.permutation(np.linspace(-2.0, 2.0, 1100)), pick):
        hd, cy, cx, a = cells[k]
        t = heads[hd][2, cy, cx, a]
        t[0:2] = rng.uniform(-2, 2, 2)
        t[2:4] = -6.0
        t[4] = 12.0
        t[5] = tc
    return [h.reshape(h.shape[0], h.shape[1], h.shape[2], 255) for h in heads]


def unmap_boxes(h2, w2, ox, oy, S_h, S_w):
    """-> (boxes f32[UNMAP_B,UNMAP_MAX_DET,4] in letterbox pixels with the sentinel in every row at or beyond UNMAP_COUNTS[b],
    {kind: rows of frame 0}).  Frame 0 holds the sixteen crafted rows, frame 1 none, frame 2 the rows 5..9 (the four padding
    bars and the box on the image's own corners)."""
    L, R, T, Bt = float(ox), float(ox + w2), float(oy), float(oy + h2)
    rng = np.random.default_rng(17)
    rows = [
        (L + 0.25 * w2, T + 0.25 * h2, L + 0.75 * w2, T + 0.625 * h2),      # 0     inside the image
        (L - 3.5, T + 1, L + 2.25, Bt - 1),                                  # 1-4   straddling the left, right, top, bottom edge
        (R - 2.5, T + 0.5, R + 4, Bt - 0.5),
        (L + 1, T - 2.75, R - 1, T + 3),
        (L + 1, Bt - 1.5, R - 1, Bt + 6),
        (L - 9, T, L - 2, Bt),                                               # 5-8   wholly inside the left, right, top, bottom bar
        (R + 1, T, R + 7.5, Bt),
        (L, T - 8, R, T - 0.5),
        (L, Bt + 0.5, R, Bt + 5),
        (L, T, R, Bt),                                                       # 9     corners exactly on ox, oy, ox + w', oy + h'
        (-17.25, -3.5, -1, -0.125),                                          # 10    negative coordinates
        (-1e30, -1e30, 1e30, 1e30),                                          # 11-12 +-1e30
        (1e30, -1e30, -1e30, 1e30),
    ]
    for _ in range(UNMAP_MAX_DET - len(rows)):                               # 13-15 anywhere on the canvas, fractional
        x, y = np.sort(rng.uniform(0, S_w, 2)), np.sort(rng.uniform(0, S_h, 2))
        rows.append((x[0], y[0], x[1], y[1]))
    rows = np.array(rows, np.float32)
    assert rows.shape == (UNMAP_MAX_DET, 4) and np.isfinite(rows).all()
    boxes = np.full((UNMAP_B, UNMAP_MAX_DET, 4), UNMAP_SENTINEL, np.float32)
    boxes[0] = rows
    boxes[2, :UNMAP_COUNTS[2]] = rows[5:5 + UNMAP_COUNTS[2]]
    kinds = {"inside": [0], "straddle": [1, 2, 3, 4], "bar_x": [5, 6], "bar_y": [7, 8], "corners": [9]}
    return boxes, kinds


# ---- heads for the post-processing's edges ----------------------------------------------------------------------------------------
# A cell is named (head 0..2, anchor 0..2, cy, cx).  With tx = ty = tw = th = 0 its box is exact in every arithmetic: the centre is
# (c + 0.5) * stride, the size the anchor's.  Head 0 (stride 32, grid 4 x 5 at POST_SIZE), anchor 0 (116 x 90), row 1: cells one
# column apart overlap 84 x 90 = 7560 of a union of 13320, cells two columns apart 52 x 90 = 4680 of 16200.
EDGE_IOU_1 = np.float32(7560) / np.float32(13320)
EDGE_IOU_2 = np.float32(4680) / np.float32(16200)
EDGE_A, EDGE_B, EDGE_C = (0, 0, 1, 0), (0, 0, 1, 1), (0, 0, 1, 2)
# a head-16 cell (anchor 2, 59 x 119, centre (40, 40)) that overlaps EDGE_B (centre (48, 48)) by 59 x 90 = 5310 of 12151
EDGE_B16 = (1, 2, 2, 2)
# anchors 0 (30 x 61) and 1 (62 x 45) of one head-16 cell overlap 30 x 45 = 1350 of 3270
EDGE_ANCHOR_PAIR = ((1, 0, 4, 5), (1, 1, 4, 5))


def flat_index(cell, S_h=POST_SIZE[0], S_w=POST_SIZE[1]):
    hd, a, cy, cx = cell
    gs = grids(S_h, S_w)
    return sum(3 * gh * gw for gh, gw in gs[:hd]) + (a * gs[hd][0] + cy) * gs[hd][1] + cx


def edge_heads(cells, B=1, S_h=POST_SIZE[0], S_w=POST_SIZE[1]):
    """Head tensors f32[B,gh,gw,255] whose background is crafted_heads' (objectness logit -8: 3e-4; class 0 wins) and whose
    named cells are set: cells = {(head, anchor, cy, cx): {"box": (tx, ty, tw, th), "to": .., "tc0": .., "frame": ..}}, every key
    optional: box zeros, to = 0 (objectness exactly 0.5), tc0 = 0 (score exactly 0.25), the other classes -2, frame = all."""
    heads = [np.zeros((B, gh, gw, 3, 85), np.float32) for gh, gw in grids(S_h, S_w)]
    for h in heads:
        h[..., 4] = -8.0
        h[..., 5] = 2.0
        h[..., 6:] = -2.0
    for (hd, a, cy, cx), spec in cells.items():
        t = heads[hd][spec.get("frame", slice(None)), cy, cx, a]
        t[..., 0:4] = spec.get("box", (0, 0, 0, 0))
        t[..., 4] = spec.get("to", 0.0)
        t[..., 5] = spec.get("tc0", 0.0)
        t[..., 6:] = np.minimum(-2.0, t[..., 5:6] - 1.0)
    return [h.reshape(B, h.shape[1], h.shape[2], 255) for h in heads]


def all_cells(S_h=POST_SIZE[0], S_w=POST_SIZE[1]):
    """Every cell (head, anchor, cy, cx) in flat order."""
    return [(hd, a, cy, cx) for hd, (gh, gw) in enumerate(grids(S_h, S_w)) for a in range(3) for cy in range(gh) for cx in range(gw)]


def cut_heads(n, tie=False, seed=4):
    """n candidates at POST_SIZE with boxes below a pixel (tw = th = -6, tx = ty = 0) and scores on a grid (tc0 on n values 4 / n
    apart in -2..2: scores at least 1e-4 apart, dealt to the cells at random).  tie: the two lowest scores are made equal, so
    that only the flat index orders the candidates at ranks n - 2 and n - 1.  -> (heads, the cells in the order dealt)."""
    rng = np.random.default_rng(seed)
    cells = all_cells()
    pick = [cells[k] for k in rng.permutation(len(cells))[:n]]
    tc = np.linspace(2.0, -2.0, n)
    if tie:
        tc[-1] = tc[-2]
    tc = tc[rng.permutation(n)]
    return edge_heads({c: {"box": (0, 0, -6, -6), "tc0": float(v)} for c, v in zip(pick, tc)}), pick
