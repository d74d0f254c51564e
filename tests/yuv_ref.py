"""The YUV4MPEG2 contract of include/poserisk_hip.h (section j6) restated in numpy: the stream syntax, the chroma taps at a
scale of 16, the matrix integers and the integer conversion.  What pr_y4m_parse_header, pr_y4m_index, pr_yuv_plan and
pr_yuv_frames are compared with, bit for bit; `convert_f64` is the float64 evaluation of the same taps with the exact matrix,
which the contract must stay within one level of."""
import numpy as np

CHROMAS = ("420jpeg", "420mpeg2", "422", "444", "mono")            # index = PR_Y4M_C*
C_FIELD = {"420jpeg": 0, "420mpeg2": 1, "420": 0, "422": 2, "444": 3, "mono": 4}
MATRICES = {"601": (0.299, 0.114), "709": (0.2126, 0.0722)}        # index in sorted order = PR_YUV_*
FULL, CENTRED, COSITED = 0, 1, 2
AXES = {"420jpeg": (CENTRED, CENTRED), "420mpeg2": (COSITED, CENTRED), "422": (COSITED, FULL), "444": (FULL, FULL)}   # (x, y)
MAX_SIDE = 4096


def chroma_size(W, H, chroma):
    """-> (cw, ch); (0, 0) for mono."""
    if chroma == "mono":
        return 0, 0
    return ((W + 1) // 2 if chroma in ("420jpeg", "420mpeg2", "422") else W), ((H + 1) // 2 if chroma in ("420jpeg", "420mpeg2") else H)


def frame_bytes(W, H, chroma):
    cw, ch = chroma_size(W, H, chroma)
    return W * H + 2 * cw * ch


def parse_header(data):
    """-> dict(width, height, fps_num, fps_den, chroma (name), full_range (True | False | None), header_bytes, frame_bytes), or
    raises ValueError with the refusal's key word."""
    data = bytes(data[:1024])
    if data[:9] != b"YUV4MPEG2"[:len(data[:9])]:
        raise ValueError("signature")
    end = data.find(b"\n", 9)
    if end < 0:
        raise ValueError("header")
    if end > 9 and data[9:10] != b" ":
        raise ValueError("signature")
    o = dict(fps_num=0, fps_den=0, chroma="420jpeg", full_range=None)
    W = H = None
    for tok in data[9:end].split(b" "):
        if not tok:
            continue
        tag, val = tok[:1], tok[1:].decode("latin-1")
        number = lambda s: int(s) if s.isascii() and s.isdigit() and len(s) <= 9 else None
        if tag in (b"W", b"H"):
            if number(val) is None:
                raise ValueError("field")
            if tag == b"W":
                W = number(val)
            else:
                H = number(val)
        elif tag == b"F":
            num, _, den = val.partition(":")
            if number(num) is None or number(den) is None or (number(den) == 0 and number(num) != 0):
                raise ValueError("field")
            o["fps_num"], o["fps_den"] = number(num), number(den)
        elif tag == b"I":
            if val in ("t", "b", "m"):
                raise ValueError("interlaced")
            if val not in ("p", "?"):
                raise ValueError("field")
        elif tag == b"C":
            if val in C_FIELD:
                o["chroma"] = CHROMAS[C_FIELD[val]]
            elif val == "420paldv":
                raise ValueError("paldv")
            elif val == "444alpha":
                raise ValueError("alpha")
            elif val == "411":
                raise ValueError("4:1:1")
            else:
                for base in ("420", "422", "444", "mono"):
                    rest = val[len(base):]
                    rest = rest[1:] if rest[:1] == "p" else rest
                    if val.startswith(base) and len(val) > len(base) and number(rest) is not None and number(rest) > 8:
                        raise ValueError("8 bits")
                raise ValueError("unknown chroma")
        elif tag == b"X":
            if val == "COLORRANGE=FULL":
                o["full_range"] = True
            if val == "COLORRANGE=LIMITED":
                o["full_range"] = False
    if W is None or H is None:
        raise ValueError("no W or no H")
    if not (1 <= W <= MAX_SIDE and 1 <= H <= MAX_SIDE):
        raise ValueError("side")
    if o["fps_den"] == 0:
        o["fps_num"] = 0
    o.update(width=W, height=H, header_bytes=end + 1, frame_bytes=frame_bytes(W, H, o["chroma"]))
    return o


def index(data, info, max_frames=1 << 30):
    """data begins at a FRAME header -> (payload offsets of the complete frames, bytes consumed); ValueError("frame k") where
    no FRAME header begins."""
    data = bytes(data)
    pos, offsets = 0, []
    while len(offsets) < max_frames and pos < len(data):
        head = data[pos:pos + 256]
        if head[:5] != b"FRAME"[:len(head[:5])] or (len(head) > 5 and head[5:6] not in (b" ", b"\n")):
            raise ValueError(f"frame {len(offsets)}")
        end = head.find(b"\n", 5)
        if end < 0:
            if len(head) < 256:
                break
            raise ValueError(f"frame {len(offsets)}")
        payload = pos + end + 1
        if len(data) - payload < info["frame_bytes"]:
            break
        offsets.append(payload)
        pos = payload + info["frame_bytes"]
    return offsets, pos


def planes_of(data, offset, W, H, chroma):
    """-> (Y u8[H,W], U, V u8[ch,cw] or None, None) of the payload at `offset`."""
    a = np.frombuffer(bytes(data), np.uint8)
    cw, ch = chroma_size(W, H, chroma)
    Y = a[offset:offset + W * H].reshape(H, W)
    if chroma == "mono":
        return Y, None, None
    U = a[offset + W * H:offset + W * H + cw * ch].reshape(ch, cw)
    V = a[offset + W * H + cw * ch:offset + W * H + 2 * cw * ch].reshape(ch, cw)
    return Y, U, V


def axis_taps(kind, S, size):
    """-> (i0, i1, w0, w1), arrays over the S full-resolution samples of an axis whose plane has `size` samples."""
    pos = np.arange(S)
    if kind == FULL:
        return pos, pos, np.full(S, 4), np.zeros(S, np.int64)
    i, odd = pos >> 1, (pos & 1) == 1
    up, down = np.minimum(i + 1, size - 1), np.maximum(i - 1, 0)
    if kind == CENTRED:
        return i, np.where(odd, up, down), np.full(S, 3), np.ones(S, np.int64)
    return i, np.where(odd, up, i), np.where(odd, 2, 4), np.where(odd, 2, 0)


def chroma16(plane, W, H, chroma):
    """C16 int64[..., H, W] of a chroma plane [..., ch, cw]."""
    xk, yk = AXES[chroma]
    ch, cw = plane.shape[-2:]
    x0, x1, a0, a1 = axis_taps(xk, W, cw)
    y0, y1, b0, b1 = axis_taps(yk, H, ch)
    c = plane.astype(np.int64)
    rows = c[..., :, x0] * a0 + c[..., :, x1] * a1
    return rows[..., y0, :] * b0[:, None] + rows[..., y1, :] * b1[:, None]


def scales(full_range):
    return (1.0, 1.0, 0) if full_range else (255.0 / 219.0, 255.0 / 224.0, 16)


def plan(matrix, full_range):
    """-> (cy, crv, cbu, cgu, cgv, yo): pr_yuv_plan's integers."""
    kr, kb = MATRICES[matrix]
    kg = 1.0 - kr - kb
    sy, sc, yo = scales(full_range)
    r = lambda v: int(np.rint(v * 65536.0))
    return r(sy), r(2 * (1 - kr) * sc), r(2 * (1 - kb) * sc), r(2 * kb * (1 - kb) / kg * sc), r(2 * kr * (1 - kr) / kg * sc), yo


def _yuv16(Y, U, V, chroma):
    H, W = Y.shape[-2:]
    if chroma == "mono":
        z = np.full(Y.shape, 2048, np.int64)
        return z, z
    return chroma16(U, W, H, chroma), chroma16(V, W, H, chroma)


def convert(Y, U, V, chroma, matrix="601", full_range=False, bgr=False, return_sums=False):
    """Planes [..., H, W] / [..., ch, cw] -> u8[..., H, W, 3] by the contract, in int64 with the int32 range asserted."""
    cy, crv, cbu, cgu, cgv, yo = plan(matrix, full_range)
    U16, V16 = _yuv16(Y, U, V, chroma)
    y, u, v = 16 * (Y.astype(np.int64) - yo), U16 - 2048, V16 - 2048
    sums = np.stack([cy * y + crv * v + (1 << 19), cy * y - cgu * u - cgv * v + (1 << 19), cy * y + cbu * u + (1 << 19)], -1)
    assert np.abs(sums).max() < 2 ** 31
    for part in (cy * y, crv * v, cgu * u, cgv * v, cbu * u, cy * y - cgu * u):
        assert np.abs(part).max() < 2 ** 31
    if return_sums:
        return sums
    rgb = np.clip(sums >> 20, 0, 255).astype(np.uint8)
    return rgb[..., ::-1].copy() if bgr else rgb


def convert_f64(Y, U, V, chroma, matrix="601", full_range=False):
    """The same taps and the exact matrix in float64, unrounded and unclamped: float64[..., H, W, 3] (RGB)."""
    kr, kb = MATRICES[matrix]
    kg = 1.0 - kr - kb
    sy, sc, yo = scales(full_range)
    U16, V16 = _yuv16(Y, U, V, chroma)
    y = (Y.astype(np.float64) - yo) * sy
    u, v = (U16 / 16.0 - 128.0) * sc, (V16 / 16.0 - 128.0) * sc
    return np.stack([y + 2 * (1 - kr) * v, y - 2 * kb * (1 - kb) / kg * u - 2 * kr * (1 - kr) / kg * v, y + 2 * (1 - kb) * u], -1)


def decode(data, matrix="601", full_range=None, bgr=False):
    """A whole stream -> (u8[F,H,W,3], info); full_range None takes the header's (limited when it says nothing)."""
    info = parse_header(data)
    offsets, used = index(data[info["header_bytes"]:], info)
    if info["header_bytes"] + used != len(data):
        raise ValueError(f"frame {len(offsets)} is incomplete")
    full = bool(info["full_range"]) if full_range is None else bool(full_range)
    W, H, c = info["width"], info["height"], info["chroma"]
    frames = [convert(*planes_of(data, info["header_bytes"] + o, W, H, c), c, matrix, full, bgr) for o in offsets]
    return (np.stack(frames) if frames else np.zeros((0, H, W, 3), np.uint8)), info
