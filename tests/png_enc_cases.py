"""The PNG encoder's cases for the CPU, native and GPU suites: dict(name, px u8[H,W,3] RGB, filter 0..5, mode).  Everything
comes from integer arithmetic or a seeded generator, so the arrays are the same everywhere.  Sizes are written W x H."""
import functools

import numpy as np

import png_enc_ref as ref

SIZES = ((1, 1), (5, 3), (21, 16), (64, 40), (85, 64), (85, 65), (683, 9), (160, 90))
# 64 x 40: 7 720 filtered bytes, less than a segment.  85 x 64: 64 (1 + 255) = 16 384, exactly one segment; 85 x 65 adds a
# second of 256 bytes.  683 x 9: rows of 2 050 bytes, two segments, the boundary at column 2 034 of row 7.
RUN_LENGTHS = (1, 2, 3, 4, 258, 259, 260, 261, 262, 517)
FIBONACCI = (1, 1, 2, 3, 5, 8, 13, 21, 34, 55, 89, 144, 233, 377, 610, 987, 1597, 2584, 4181)


def smooth(W, H, seed=0):
    """A smooth picture with two bits of noise."""
    y, x = np.mgrid[0:H, 0:W].astype(np.int64)
    h = ((x * 73856093) ^ (y * 19349663) ^ ((x * y + seed) * 83492791)) >> 5
    return np.stack([(x * 255 // max(W - 1, 1) + (h & 3)) & 255, (y * 255 // max(H - 1, 1) + ((h >> 3) & 3)) & 255,
                     ((x + 2 * y) * 255 // max(W + 2 * H - 3, 1) + ((h >> 6) & 3)) & 255], -1).astype(np.uint8)


def noise(W, H, seed=1):
    return np.random.default_rng(seed * 7919 + W * 31 + H).integers(0, 256, (H, W, 3), dtype=np.uint8)


def canvas():
    """u8[450,1000,3] shaped like a composed score canvas: a smooth and noisy photo area 720 px wide, then a black panel with
    a little text."""
    img = np.zeros((450, 1000, 3), np.uint8)
    img[:, :720] = smooth(720, 450, seed=5)
    img[:, :720] += np.random.default_rng(11).integers(0, 6, (450, 720, 3), dtype=np.uint8)
    y, x = np.mgrid[0:450, 0:1000]
    text = (x >= 730) & (y % 18 < 11) & (((x * 7 + y // 18 * 13) % 11) < 3) & (x % 140 > 12) & (y < 200)
    img[text] = 255
    return img


def _row(values):
    """One row of pixels whose raw bytes are `values` (a multiple of three of them)."""
    v = np.asarray(values, np.uint8)
    assert v.size % 3 == 0
    return v.reshape(1, -1, 3)


def runs_row():
    """Filter 0, one row of 4096 pixels: behind the type byte, runs of exactly RUN_LENGTHS equal bytes, each of another
    value, then bytes that never repeat."""
    v = []
    for k, n in enumerate(RUN_LENGTHS):
        v += [10 + k] * n
    v += [(i % 251) + 1 for i in range(3 * 4096 - len(v))]
    assert v[sum(RUN_LENGTHS)] != v[sum(RUN_LENGTHS) - 1]
    return _row(v)


def crossing():
    """683 x 9 noise with a run of one value from byte 16 251 to 16 399 of the filtered stream: across the boundary at 16 384."""
    px = noise(683, 9, seed=3).reshape(9, 2049)
    px[7, 1900:] = 77
    return px.reshape(9, 683, 3)


def no_match():
    """64 x 40 of thirteen values, none of them 0 (the type bytes are), no two neighbours equal: no match anywhere, and a
    dynamic block that is smaller than the stored one."""
    return ((np.arange(40 * 64 * 3, dtype=np.int64) * 37 + 11) % 13 + 1).astype(np.uint8).reshape(40, 64, 3)


@functools.lru_cache(maxsize=None)
def fibonacci_row():
    """Filter 0, one row of 3648 pixels: with the type byte (the one 0) the segment's 10 945 bytes have 19 values whose counts
    are FIBONACCI; no two neighbours are equal, so there is no match and the histogram is the byte histogram."""
    left = {20 + k: n for k, n in enumerate(FIBONACCI) if k}
    v, prev = [], 0
    while left:
        s = max((s for s in left if s != prev), key=lambda s: (left[s], s))
        v.append(s)
        prev = s
        left[s] -= 1
        if not left[s]:
            del left[s]
    assert len(v) == 10944
    return _row(v)


def two_values():
    """Filter 0, one row of 1000 pixels: 0 (type), 7, 0, 7, ...: exactly two literal values and no run."""
    return _row([7, 0] * 1500)


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    add = lambda name, px, filt=ref.ADAPTIVE, mode=ref.RLE: out.append(
        dict(name=f"{name}_f{filt}_{'rle' if mode else 'stored'}", px=np.ascontiguousarray(px), filter=filt, mode=mode))
    for W, H in SIZES:
        add(f"{W}x{H}_zero", np.zeros((H, W, 3), np.uint8))
        add(f"{W}x{H}_255", np.full((H, W, 3), 255, np.uint8))
        add(f"{W}x{H}_noise", noise(W, H))
        add(f"{W}x{H}_smooth", smooth(W, H))
    for W, H in ((21, 16), (683, 9)):
        for filt in range(5):
            add(f"{W}x{H}_smooth", smooth(W, H), filt)
        add(f"{W}x{H}_noise", noise(W, H), 0)
        add(f"{W}x{H}_smooth", smooth(W, H), 0, ref.STORED)
        add(f"{W}x{H}_smooth", smooth(W, H), ref.ADAPTIVE, ref.STORED)
    add("4096x1_runs", runs_row(), 0)
    add("683x9_crossing", crossing(), 0)
    add("64x40_nomatch", no_match(), 0)
    add("3648x1_fibonacci", fibonacci_row(), 0)
    add("1000x1_two_values", two_values(), 0)
    return out


@functools.lru_cache(maxsize=None)
def reference(name):
    """The reference's file for a case and what it noted on the way: computed once, shared by every test."""
    c = next(c for c in cases() if c["name"] == name)
    info = {}
    return ref.encode(c["px"], c["filter"], c["mode"], info), info
