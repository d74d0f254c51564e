"""YUV4MPEG2 streams for the tests of the reader (include/poserisk_hip.h, section j6): builders, the accepted headers, and
every refusal with the word its name must contain.  Pure Python + numpy."""
import numpy as np

import yuv_ref

SIZES = ((1, 1), (2, 3), (3, 2), (5, 7), (7, 5), (37, 53), (53, 37))     # (W, H)
# FRAME headers without and with fields, one per length modulo 4: stream() picks for frame k the one that puts its payload at
# byte alignment k % 4 of the stream, so four frames cover all four
FRAME_FIELDS = (b"", b" Xabc", b" X", b" Ip")
# the C field as written -> the layout it means (None: no C field)
ACCEPTED_C = ((None, "420jpeg"), ("420jpeg", "420jpeg"), ("420mpeg2", "420mpeg2"), ("420", "420jpeg"), ("422", "422"), ("444", "444"),
              ("mono", "mono"))
RANGES = ((None, None), ("FULL", True), ("LIMITED", False))         # XCOLORRANGE as written -> full_range


def planes(W, H, chroma, F=1, seed=0, kind="noise"):
    """-> (Y u8[F,H,W], U, V u8[F,ch,cw] or None): noise over the whole byte range, or `extreme`: 0 / 255 only."""
    rng = np.random.default_rng(seed)
    cw, ch = yuv_ref.chroma_size(W, H, chroma)
    draw = (lambda *s: rng.integers(0, 256, s, dtype=np.uint8)) if kind == "noise" else \
        (lambda *s: (255 * rng.integers(0, 2, s)).astype(np.uint8))
    Y = draw(F, H, W)
    if chroma == "mono":
        return Y, None, None
    return Y, draw(F, ch, cw), draw(F, ch, cw)


def header(W, H, c_field=None, fps=(25, 1), interlace=None, aspect=None, colorrange=None, extra=()):
    parts = [b"YUV4MPEG2", b"W%d" % W, b"H%d" % H]
    if fps is not None:
        parts.append(b"F%d:%d" % tuple(fps))
    if interlace is not None:
        parts.append(b"I" + interlace.encode())
    if aspect is not None:
        parts.append(b"A" + aspect.encode())
    if c_field is not None:
        parts.append(b"C" + c_field.encode())
    if colorrange is not None:
        parts.append(b"XCOLORRANGE=" + colorrange.encode())
    parts += [e if isinstance(e, bytes) else e.encode() for e in extra]
    return b" ".join(parts) + b"\n"


def stream(Y, U, V, head, frame_fields=FRAME_FIELDS):
    """The planes' frames behind `head`, frame k's payload at alignment k % 4 (with one field set given: that one throughout)
    -> (bytes, payload offsets)."""
    out, offsets = bytearray(head), []
    for k in range(Y.shape[0]):
        fields = [f for f in frame_fields if (len(out) + 6 + len(f)) % 4 == k % 4] or list(frame_fields)
        out += b"FRAME" + fields[0] + b"\n"
        offsets.append(len(out))
        out += Y[k].tobytes()
        if U is not None:
            out += U[k].tobytes() + V[k].tobytes()
    return bytes(out), offsets


def case(W, H, chroma, F=5, seed=0, colorrange=None, kind="noise", **head):
    """-> (stream bytes, offsets, (Y, U, V)): F frames whose payloads start at alignments 0, 1, 2, 3, 0, ... of the stream."""
    c_field = head.pop("c_field", chroma)
    Y, U, V = planes(W, H, chroma, F, seed, kind)
    data, offsets = stream(Y, U, V, header(W, H, c_field, colorrange=colorrange, **head))
    return data, offsets, (Y, U, V)


def alignments(offsets):
    return {o % 4 for o in offsets}


# (stream header, the word pr_y4m_refusal_name's text must contain, the PR_Y4M_E_* name)
REFUSALS = (
    (b"YUV4MPEG W4 H4\n", "signature", "MAGIC"),
    (b"RIFF\0\0\0\0AVI LIST", "signature", "MAGIC"),
    (b"YUV4MPEG2W4 H4\n", "signature", "MAGIC"),
    (b"YUV4MPEG2 W4 H4 " + b"Xpad " * 300 + b"\n", "does not end within 1024", "HEADER"),
    (b"YUV4MPEG2 W4 H4", "does not end within 1024", "HEADER"),
    (b"YUV4", "does not end within 1024", "HEADER"),
    (b"YUV4MPEG2 W4x H4\n", "malformed", "FIELD"),
    (b"YUV4MPEG2 W H4\n", "malformed", "FIELD"),
    (b"YUV4MPEG2 W4 H4 F25\n", "malformed", "FIELD"),
    (b"YUV4MPEG2 W4 H4 F25:0\n", "malformed", "FIELD"),
    (b"YUV4MPEG2 W4 H4 Iq\n", "malformed", "FIELD"),
    (b"YUV4MPEG2 W4 H4 Ipp\n", "malformed", "FIELD"),
    (b"YUV4MPEG2 H4 F25:1\n", "no W or no H", "NO_SIZE"),
    (b"YUV4MPEG2 W4\n", "no W or no H", "NO_SIZE"),
    (b"YUV4MPEG2\n", "no W or no H", "NO_SIZE"),
    (b"YUV4MPEG2 W0 H4\n", "outside 1..4096", "SIZE"),
    (b"YUV4MPEG2 W4 H4097\n", "outside 1..4096", "SIZE"),
    (b"YUV4MPEG2 W4 H4 It\n", "interlaced", "INTERLACED"),
    (b"YUV4MPEG2 W4 H4 Ib\n", "interlaced", "INTERLACED"),
    (b"YUV4MPEG2 W4 H4 Im\n", "interlaced", "INTERLACED"),
    (b"YUV4MPEG2 W4 H4 C420paldv\n", "420paldv", "PALDV"),
    (b"YUV4MPEG2 W4 H4 C420p10\n", "more than 8 bits", "HIGH_DEPTH"),
    (b"YUV4MPEG2 W4 H4 C420p12\n", "more than 8 bits", "HIGH_DEPTH"),
    (b"YUV4MPEG2 W4 H4 C422p10\n", "more than 8 bits", "HIGH_DEPTH"),
    (b"YUV4MPEG2 W4 H4 C422p14\n", "more than 8 bits", "HIGH_DEPTH"),
    (b"YUV4MPEG2 W4 H4 C444p16\n", "more than 8 bits", "HIGH_DEPTH"),
    (b"YUV4MPEG2 W4 H4 Cmono16\n", "more than 8 bits", "HIGH_DEPTH"),
    (b"YUV4MPEG2 W4 H4 C411\n", "4:1:1", "411"),
    (b"YUV4MPEG2 W4 H4 C444alpha\n", "444alpha", "ALPHA"),
    (b"YUV4MPEG2 W4 H4 C440\n", "unknown chroma", "CHROMA"),
    (b"YUV4MPEG2 W4 H4 C420jpegx\n", "unknown chroma", "CHROMA"),
)
CODES = {"OK": 0, "MAGIC": 1, "HEADER": 2, "FIELD": 3, "NO_SIZE": 4, "SIZE": 5, "INTERLACED": 6, "PALDV": 7, "HIGH_DEPTH": 8, "411": 9,
         "ALPHA": 10, "CHROMA": 11, "FRAME": 12}
