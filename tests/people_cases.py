"""Inputs for pr_compose_people that tests/test_people_native.py (the kernel source on the host) and tests/test_people_gpu.py share:
hand-placed boxes and tags for every clause of the contract (include/poserisk_hip.h, section r3), random panel lines."""
import numpy as np

from poserisk_release_amd import video

# (W, H, dst_w, dst_h, panel_w): tap counts 2 and 3 with ragged band ends, twice; one upsampling case (one tap)
SIZES = [(37, 23, 20, 13, 24), (64, 48, 45, 34, 40), (16, 12, 40, 30, 9)]
# (K, L, L_img): panel lines only; tags only; the most of everything
SHAPES = [(2, 8, 0), (5, 12, 12), (16, 32, 16)]
NO_FRAME = 7            # a src_idx outside the case's 3 frames


def noise_atlas():
    """A small atlas of noise (cells of 11 x 7): every coverage value, no glyph shapes to hide an indexing slip."""
    cov = np.random.default_rng(5).integers(0, 256, (3, 96, 11, 7), dtype=np.uint8)
    return video.Atlas(cov, (7, 5, 3), (9, 4, 0))


def box_pool(W, H, rng):
    """16 boxes: two that overlap (the later one wins where they cross), no box (x_max < x_min), one across the left, right and
    bottom edges, one wholly off the frame, one across the top edge, then random ones (some off the frame, some inverted)."""
    pool = [(5, 4, W - 9, H - 7), (8, 6, W - 5, H - 3), (0, 0, -1, -1), (-6, H // 2, W + 3, H + 2), (W + 4, 2, W + 40, 9),
            (3, -4, W // 2, 5)]
    while len(pool) < 16:
        x0, y0 = int(rng.integers(-8, W)), int(rng.integers(-8, H))
        pool.append((x0, y0, x0 + int(rng.integers(-2, W)), y0 + int(rng.integers(0, H))))
    return np.array(pool, np.int32)


def case(size, shape, seed, atlas=None, N=4, reduction=False):
    """-> dict of pr_compose_people's arguments (numpy).  Canvas n's slot k holds pool box (k + 2 n) mod 16, so that every kind
    of box meets every slot position over the canvases, the empty one a middle slot of canvas 0 when K = 5 or 16.  The last
    canvas names a frame that does not exist.  reduction: K = 1, L_img = 0, in-range frames -- pr_compose_video's case."""
    W, H, dst_w, dst_h, panel_w = size
    K, L, L_img = (1, shape[1], 0) if reduction else shape
    atlas = atlas or noise_atlas()
    rng = np.random.default_rng(seed)
    frames = rng.integers(0, 256, (3, H, W, 3), dtype=np.uint8)
    src_idx = np.array([2, 0, 1, NO_FRAME][:N] if not reduction else [2, 0, 1][:N], np.int32)
    N = len(src_idx)
    pool = box_pool(W, H, rng)
    box = np.stack([pool[(np.arange(K) + 2 * n) % 16] for n in range(N)]).astype(np.int32)
    box_rgb = rng.integers(0, 256, (N, K, 4), dtype=np.uint8)
    S, _, CH, CW = atlas.cov.shape
    C = 9
    lines = np.zeros((N, L, 5), np.int32)
    lines[..., 2] = rng.integers(-1, S + 1, (N, L))                # with classes that do not exist
    lines[..., 3] = rng.integers(-1, C + 4, (N, L))                # with empty lines and lengths beyond C
    lines[..., 4] = rng.integers(0, 1 << 24, (N, L))
    # tags anywhere over the image and around it, panel lines anywhere over the panel and around it
    lines[:, :L_img, 0] = rng.integers(-3 * CW, dst_w + 4, (N, L_img))
    lines[:, L_img:, 0] = rng.integers(dst_w - 3 * CW, dst_w + panel_w + 4, (N, L - L_img))
    lines[..., 1] = rng.integers(-3, dst_h + CH + 3, (N, L))
    if L_img >= 5:
        a = atlas.adv[0]
        sx, sy = pool[0][0] * dst_w // W, pool[0][1] * dst_h // H
        placed = [(-a - 2, dst_h // 2, 6),                          # starts left of x = 0
                  (dst_w - 2 * a - 1, dst_h // 3, 7),               # runs across the image / panel boundary: clipped at dst_w
                  (dst_w // 4, dst_h - 2, 5), (dst_w // 4 + 2, dst_h - 1, 5),      # two tags that overlap each other
                  (sx, sy + atlas.ascent[0] - 1, 4)]                # sits on a box outline (pool box 0: canvas 0's slot 0)
        for l, (x, yb, length) in enumerate(placed):
            lines[:, l, :4] = (x, yb, 0, length)
    text = rng.integers(0, 256, (N, L, C), dtype=np.uint8)         # half the codes outside 32..127
    text[:, :5] = rng.integers(33, 127, (N, min(5, L), C), dtype=np.uint8)
    return dict(frames=frames, src_idx=src_idx, box=box, box_rgb=box_rgb, lines=lines, text=text, L_img=L_img, atlas=atlas,
                dst_h=dst_h, dst_w=dst_w, panel_w=panel_w)


def reference(c, canvases=None):
    import video_people_ref as pref
    a = c["atlas"]
    return pref.compose_people(c["frames"], c["src_idx"], c["box"], c["box_rgb"], c["lines"], c["text"], c["L_img"], np.asarray(a.cov),
                               a.adv, a.ascent, c["dst_h"], c["dst_w"], c["panel_w"], canvases)
