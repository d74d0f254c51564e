"""The compose contract of include/poserisk_hip.h (pr_compose_video) restated in numpy: box, area resample, panel text.  Written
from the contract's text, not from csrc/compose.hip; it is the only oracle for the canvases' pixels
(tests/test_video_gpu.py compares every byte, tests/test_video_cpu.py checks the resample against a float64 formulation)."""
import numpy as np


def draw_box(img, box, rgb):
    """img u8[H,W,3], box (x_min, y_min, x_max, y_max) -> a copy with the outline: pixels inside
    [x_min-1, x_max+1] x [y_min-1, y_max+1] and not inside [x_min+2, x_max-2] x [y_min+2, y_max-2], clipped to the frame.
    x_max < x_min: no box."""
    img = np.array(img, np.uint8)
    x0, y0, x1, y1 = (int(v) for v in box)
    if x1 < x0:
        return img
    H, W = img.shape[:2]
    ys, xs = np.mgrid[0:H, 0:W]
    outer = (xs >= x0 - 1) & (xs <= x1 + 1) & (ys >= y0 - 1) & (ys <= y1 + 1)
    inner = (xs >= x0 + 2) & (xs <= x1 - 2) & (ys >= y0 + 2) & (ys <= y1 - 2)
    img[outer & ~inner] = np.asarray(rgb, np.uint8)[:3]
    return img


def overlaps(n_src, n_dst):
    """int64[n_dst, n_src]: the overlap of destination cell i = [i n_src, (i+1) n_src) with source cell j =
    [j n_dst, (j+1) n_dst), in units of 1 / (n_src n_dst).  Every row sums to n_src."""
    i = np.arange(n_dst, dtype=np.int64)[:, None]
    j = np.arange(n_src, dtype=np.int64)[None, :]
    return np.maximum(0, np.minimum((j + 1) * n_dst, (i + 1) * n_src) - np.maximum(j * n_dst, i * n_src))


def area_sums(img, dst_h, dst_w):
    """S int64[dst_h,dst_w,3] = sum oy ox src, exact: the products run in float64 (for BLAS), where every partial sum is an
    integer below 2^32 and therefore exact."""
    H, W = img.shape[:2]
    oy, ox = overlaps(H, dst_h).astype(np.float64), overlaps(W, dst_w).astype(np.float64)
    rows = (oy @ np.asarray(img, np.float64).reshape(H, W * 3)).reshape(dst_h, W, 3)     # [dst_h, W, 3]
    S = np.matmul(rows.transpose(0, 2, 1), ox.T).transpose(0, 2, 1)                        # [dst_h, dst_w, 3]
    return S.astype(np.int64)


def area_resample(img, dst_h, dst_w):
    """img u8[H,W,3] -> u8[dst_h,dst_w,3]: S / (H W) rounded half to even."""
    H, W = img.shape[:2]
    S = area_sums(img, dst_h, dst_w)
    assert int(S.max(initial=0)) < 2 ** 32
    D = H * W
    q, r = np.divmod(S, D)
    q = q + ((2 * r > D) | ((2 * r == D) & (q % 2 == 1)))
    return q.astype(np.uint8)


def draw_text(canvas, x_from, lines, text, cov, adv, ascent):
    """Blend the lines over columns [x_from, width) of canvas u8[h,w,3] in place.  lines int[L,5] = (x0, yb, class, length,
    colour c0 | c1 << 8 | c2 << 16), text u8[L,C], cov u8[S,96,CH,CW]."""
    h, w = canvas.shape[:2]
    S, _, CH, CW = cov.shape
    C = text.shape[1]
    ys, xs = np.arange(h)[:, None], np.arange(x_from, w)[None, :]
    for l in range(lines.shape[0]):
        x0, yb, s, length, colour = (int(v) for v in lines[l])
        length = min(length, C)
        if not 0 <= s < S or length <= 0:
            continue
        k = (xs - x0) // adv[s]                                  # floor division
        u = (xs - x0) - k * adv[s]
        v = ys - (yb - ascent[s])
        ok = (k >= 0) & (k < length) & (v >= 0) & (v < CH)
        code = text[l][np.clip(k, 0, length - 1)].astype(np.int64)
        ok = ok & (code >= 32) & (code <= 127)
        c = cov[s][np.clip(code - 32, 0, 95), np.clip(v, 0, CH - 1), np.clip(u, 0, CW - 1)].astype(np.int64)
        region = canvas[:, x_from:]
        for ch in range(3):
            col = (colour >> (8 * ch)) & 255
            bg = region[:, :, ch].astype(np.int64)
            new = (2 * (bg * (255 - c) + col * c) + 255) // 510
            region[:, :, ch] = np.where(ok, new, bg).astype(np.uint8)


def compose(frames, src_idx, box, lines, text, cov, adv, ascent, dst_h, dst_w, panel_w, box_rgb, canvases=None):
    """-> (out u8[N,dst_h,dst_w+panel_w,3], status int32[N]); only the canvases named in `canvases` are computed (the others
    stay zero)."""
    n_frames = frames.shape[0]
    N = len(src_idx) if src_idx is not None else n_frames
    out = np.zeros((N, dst_h, dst_w + panel_w, 3), np.uint8)
    status = np.zeros(N, np.int32)
    for n in (range(N) if canvases is None else canvases):
        f = int(src_idx[n]) if src_idx is not None else n
        if 0 <= f < n_frames:
            img = frames[f] if box is None else draw_box(frames[f], box[n], box_rgb)
            out[n, :, :dst_w] = area_resample(img, dst_h, dst_w)
        else:
            status[n] = 1
        if lines is not None:
            draw_text(out[n], dst_w, lines[n], text[n], cov, adv, ascent)
    for n in range(N):
        f = int(src_idx[n]) if src_idx is not None else n
        status[n] = 0 if 0 <= f < n_frames else 1
    return out, status
