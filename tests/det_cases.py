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
