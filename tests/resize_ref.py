"""The frame downscale of include/poserisk_hip.h (section j3) restated in numpy: the per-axis tap tables, the two integer passes,
the exact-half rule and the copy.  What pr_resize_plan and pr_resize_frames are compared with, bit for bit; `bilinear_f64` is the
float64 bilinear at the same sample positions, which the contract must stay within one level of."""
import numpy as np

MODE_COPY, MODE_HALF, MODE_LINEAR = 0, 1, 2
MAX_SIDE = 4096
# (H, W) -> (h, w): the front end's two real cases, an odd pair, an upscale (the only one that reaches both clamps), the same
# size, the exact half, and a pair that is half in one axis only and must not take the half rule
PAIRS = (((1080, 1920), (450, 800)), ((480, 640), (450, 600)), ((37, 53), (17, 23)), ((19, 31), (40, 70)), ((33, 47), (33, 47)),
         ((90, 160), (45, 80)), ((90, 161), (45, 80)))
SMALL_PAIRS = PAIRS[2:]


def positions(S, d):
    """f of the contract before floor: the destination samples' positions in the source, float32."""
    scale = 1.0 / (float(d) / S)
    return ((np.arange(d, dtype=np.float64) + 0.5) * scale - 0.5).astype(np.float32)


def axis_table(S, d):
    """-> (ofs int32[d], coef int16[2 d])"""
    f = positions(S, d)
    s = np.floor(f)
    f = (f - s).astype(np.float32)
    s = s.astype(np.int64)
    low, high = s < 0, s >= S - 1
    s[low], f[low] = 0, 0
    s[high], f[high] = S - 1, 0
    c0 = np.rint((np.float32(1) - f) * np.float32(2048))
    c1 = np.rint(f * np.float32(2048))
    return s.astype(np.int32), np.stack([c0, c1], 1).astype(np.int16).reshape(-1)


def mode(H, W, h, w):
    return MODE_COPY if (H, W) == (h, w) else MODE_HALF if (W == 2 * w and H == 2 * h) else MODE_LINEAR


def plan(H, W, h, w):
    """-> (xofs, xcoef, yofs, ycoef, mode): what pr_resize_plan fills."""
    return (*axis_table(W, w), *axis_table(H, h), mode(H, W, h, w))


def linear(src, h, w):
    """The two passes on u8[..., H, W, C], whatever the sizes."""
    H, W = src.shape[-3:-1]
    xofs, xcoef, yofs, ycoef, _ = plan(H, W, h, w)
    x0, x1 = xofs, np.minimum(xofs + 1, W - 1)
    y0, y1 = yofs, np.minimum(yofs + 1, H - 1)
    a0, a1 = (xcoef.reshape(-1, 2).astype(np.int32)[:, k][:, None] for k in (0, 1))
    b0, b1 = (ycoef.reshape(-1, 2).astype(np.int32)[:, k][:, None, None] for k in (0, 1))
    s = src.astype(np.int32)
    t = s[..., :, x0, :] * a0 + s[..., :, x1, :] * a1                    # [..., H, w, C]
    t0, t1 = t[..., y0, :, :], t[..., y1, :, :]
    d = (((b0 * (t0 >> 4)) >> 16) + ((b1 * (t1 >> 4)) >> 16) + 2) >> 2
    assert d.min() >= 0 and d.max() <= 255
    return d.astype(np.uint8)


def resize(src, h, w):
    """u8[..., H, W, C] -> u8[..., h, w, C] by the contract."""
    src = np.asarray(src)
    assert src.dtype == np.uint8
    H, W = src.shape[-3:-1]
    m = mode(H, W, h, w)
    if m == MODE_COPY:
        return src.copy()
    if m == MODE_HALF:
        s = src.astype(np.int32)
        return ((s[..., 0::2, 0::2, :] + s[..., 0::2, 1::2, :] + s[..., 1::2, 0::2, :] + s[..., 1::2, 1::2, :] + 2) >> 2).astype(np.uint8)
    return linear(src, h, w)


def bilinear_f64(src, h, w):
    """The float64 bilinear interpolation at the contract's sample positions (clamped to the source), unrounded."""
    H, W = src.shape[-3:-1]

    def taps(S, d):
        f = np.clip(positions(S, d).astype(np.float64), 0, S - 1)
        s = np.minimum(np.floor(f).astype(np.int64), S - 1)
        return s, np.minimum(s + 1, S - 1), f - s
    x0, x1, fx = taps(W, w)
    y0, y1, fy = taps(H, h)
    s = src.astype(np.float64)
    fx, fy = fx[:, None], fy[:, None, None]
    t = s[..., :, x0, :] * (1 - fx) + s[..., :, x1, :] * fx
    return t[..., y0, :, :] * (1 - fy) + t[..., y1, :, :] * fy


def contents(H, W, seed=0):
    """{name: u8[H,W,3]}: noise, all-255, a 0 / 255 checker, a gradient."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    checker = np.repeat((255 * ((yy + xx) & 1)).astype(np.uint8)[..., None], 3, 2)
    gradient = np.stack([(xx * 255) // max(W - 1, 1), (yy * 255) // max(H - 1, 1), ((xx + yy) * 255) // max(W + H - 2, 1)], -1).astype(np.uint8)
    return {"noise": rng.integers(0, 256, (H, W, 3), dtype=np.uint8), "white": np.full((H, W, 3), 255, np.uint8),
            "checker": checker, "gradient": gradient}


def target_size(W, H, max_w=800, max_h=450):
    """The reference's rule (lib/utils/funcs_utils.py): -> (w, h)."""
    if max_w and W > max_w:
        return max_w, int(H * max_w / W)
    if max_h and H > max_h:
        return int(W * max_h / H), max_h
    return W, H
