"""The YUV4MPEG2 writer's contract of include/poserisk_hip.h (section j7) restated in numpy: the forward matrix's integers,
edge-replicating padding, the chroma tap sums and the one rounding a sample.  What pr_yuv_enc_plan and pr_yuv_encode are
compared with, bit for bit; `planes_f64` is the float64 evaluation of the same taps with the exact matrix, which the contract
must stay within 0.51 of."""
import numpy as np

import yuv_ref

CHROMAS = yuv_ref.CHROMAS
MATRICES = yuv_ref.MATRICES
FRAME = b"FRAME\n"


def scales(full_range):
    return (1.0, 1.0, 0) if full_range else (219.0 / 255.0, 224.0 / 255.0, 16)


def plan(matrix, full_range):
    """-> (kyr, kyg, kyb, kc, kur, kug, kvb, kvg, yo): pr_yuv_enc_plan's integers."""
    kr, kb = MATRICES[matrix]
    sy, sc, yo = scales(full_range)
    r = lambda v: int(np.rint(v))
    ky, kyr, kyb = r(sy * 65536.0), r(kr * sy * 65536.0), r(kb * sy * 65536.0)
    kc = r(sc * 32768.0)
    kur, kvb = r(kr / (2.0 * (1.0 - kb)) * sc * 65536.0), r(kb / (2.0 * (1.0 - kr)) * sc * 65536.0)
    return kyr, ky - kyr - kyb, kyb, kc, kur, kc - kur, kvb, kc - kvb, yo


def frame_bytes(out_W, out_H, chroma):
    return yuv_ref.frame_bytes(out_W, out_H, chroma)


def _padded(rgb, out_H, out_W):
    """[..., H, W, 3] -> int64 [..., out_H, out_W, 3], edge-replicated."""
    H, W = rgb.shape[-3:-1]
    assert 0 <= out_H - H <= 1 and 0 <= out_W - W <= 1
    ys, xs = np.minimum(np.arange(out_H), H - 1), np.minimum(np.arange(out_W), W - 1)
    return rgb.astype(np.int64)[..., ys, :, :][..., xs, :]


def tap_sums(rgb, chroma, out_H, out_W):
    """-> (S int64[..., ch, cw, 3]: the chroma taps' sums over the padded picture, indices clamped to it; log2 T)."""
    p = _padded(rgb, out_H, out_W)
    if chroma == "444":
        return p, 0
    cw = (out_W + 1) // 2
    i = np.arange(cw)
    col = lambda c: p[..., :, np.clip(c, 0, out_W - 1), :]
    if chroma == "420jpeg":
        rows, log_t = col(2 * i) + col(2 * i + 1), 2
    else:
        rows, log_t = col(2 * i - 1) + 2 * col(2 * i) + col(2 * i + 1), 2
    if chroma == "422":
        return rows, log_t
    j = np.arange((out_H + 1) // 2)
    return rows[..., 2 * j, :, :] + rows[..., np.minimum(2 * j + 1, out_H - 1), :, :], log_t + (chroma == "420mpeg2")


def planes(rgb, chroma="420mpeg2", matrix="601", full_range=False, bgr=False, out_size=None):
    """u8[..., H, W, 3] -> (Y u8[..., out_H, out_W], U, V u8[..., ch, cw] or None, None) by the contract, in int64 with the
    int32 range asserted.  out_size = (out_H, out_W); None: the source's."""
    rgb = np.asarray(rgb)
    if bgr:
        rgb = rgb[..., ::-1]
    out_H, out_W = out_size or rgb.shape[-3:-1]
    kyr, kyg, kyb, kc, kur, kug, kvb, kvg, yo = plan(matrix, full_range)
    p = _padded(rgb, out_H, out_W)
    Y = yo + ((kyr * p[..., 0] + kyg * p[..., 1] + kyb * p[..., 2] + (1 << 15)) >> 16)
    assert Y.min() >= 0 and Y.max() <= 255
    if chroma == "mono":
        return Y.astype(np.uint8), None, None
    S, log_t = tap_sums(rgb, chroma, out_H, out_W)
    Rs, Gs, Bs = S[..., 0], S[..., 1], S[..., 2]
    su = kc * Bs - kur * Rs - kug * Gs + (1 << (15 + log_t))
    sv = kc * Rs - kvg * Gs - kvb * Bs + (1 << (15 + log_t))
    assert max(np.abs(su).max(), np.abs(sv).max()) < 7e7
    U = np.clip(128 + (su >> (16 + log_t)), 0, 255)
    V = np.clip(128 + (sv >> (16 + log_t)), 0, 255)
    return Y.astype(np.uint8), U.astype(np.uint8), V.astype(np.uint8)


def planes_f64(rgb, chroma="444", matrix="601", full_range=False, out_size=None):
    """The same taps and the exact matrix in float64, unrounded and unclamped -> (Y, U, V)."""
    rgb = np.asarray(rgb)
    out_H, out_W = out_size or rgb.shape[-3:-1]
    kr, kb = MATRICES[matrix]
    kg = 1.0 - kr - kb
    sy, sc, yo = scales(full_range)
    p = _padded(rgb, out_H, out_W).astype(np.float64)
    Y = yo + sy * (kr * p[..., 0] + kg * p[..., 1] + kb * p[..., 2])
    if chroma == "mono":
        return Y, None, None
    S, log_t = tap_sums(rgb, chroma, out_H, out_W)
    m = S.astype(np.float64) / (1 << log_t)
    y = kr * m[..., 0] + kg * m[..., 1] + kb * m[..., 2]
    return Y, 128.0 + sc * (m[..., 2] - y) / (2.0 * (1.0 - kb)), 128.0 + sc * (m[..., 0] - y) / (2.0 * (1.0 - kr))


def encode(frames, chroma="420mpeg2", matrix="601", full_range=False, bgr=False, out_size=None):
    """u8[F,H,W,3] -> the stream bytes of a call: per frame "FRAME\\n", Y, U, V; no stream header."""
    frames = np.asarray(frames)
    Y, U, V = planes(frames, chroma, matrix, full_range, bgr, out_size)
    out = bytearray()
    for k in range(frames.shape[0]):
        out += FRAME + Y[k].tobytes()
        if U is not None:
            out += U[k].tobytes() + V[k].tobytes()
    return bytes(out)
