"""Motion-JPEG AVI files for the front-end tests, built by hand from the RIFF / AVI definition (not by the package's AviWriter):
the layouts cameras and ffmpeg write that AviWriter never does, and the damaged ones."""
import io
import struct

import numpy as np
from PIL import Image

SAMPLING = {"4:4:4": 0, "4:2:2": 1, "4:2:0": 2}


def chunk(tag, body):
    return tag + struct.pack("<I", len(body)) + body + (b"\0" if len(body) & 1 else b"")


def riff_list(kind, body):
    return chunk(b"LIST", kind + body)


def headers(width, height, n, rate=25, scale=1, us_per_frame=40000, handler=b"MJPG", compression=b"MJPG", fcc_type=b"vids",
            audio_first=False):
    """LIST 'hdrl' of one video stream (with audio_first an audio stream in front of it, so that the video is stream 01)."""
    avih = struct.pack("<14I", us_per_frame, 0, 0, 0, n, 0, 2 if audio_first else 1, 0, width, height, 0, 0, 0, 0)
    strh = struct.pack("<4s4sIHHIIIIIIiI4H", fcc_type, handler, 0, 0, 0, 0, scale, rate, 0, n, 0, -1, 0, 0, 0, width, height)
    strf = struct.pack("<IiiHH4sIiiII", 40, width, height, 1, 24, compression, width * height * 3, 0, 0, 0, 0)
    strl = riff_list(b"strl", chunk(b"strh", strh) + chunk(b"strf", strf))
    if audio_first:
        auds = struct.pack("<4s4sIHHIIIIIIiI4H", b"auds", b"\0\0\0\0", 0, 0, 0, 0, 1, 8000, 0, 0, 0, -1, 1, 0, 0, 0, 0)
        wave = struct.pack("<HHIIHH", 1, 1, 8000, 8000, 1, 8)
        strl = riff_list(b"strl", chunk(b"strh", auds) + chunk(b"strf", wave)) + strl
    return riff_list(b"hdrl", chunk(b"avih", avih) + strl)


def plain_avi(frames, width, height, tag=b"00dc", **kw):
    """RIFF 'AVI ' { hdrl, movi { one chunk per frame } }, no index."""
    movi = riff_list(b"movi", b"".join(chunk(tag, f) for f in frames))
    return chunk(b"RIFF", b"AVI " + headers(width, height, len(frames), **kw) + movi)


def foreign_avi(frames, width, height):
    """What AviWriter never writes, all at once: JUNK chunks, the video as stream 01 behind an audio stream, frames inside
    LIST 'rec ' groups with an 01wb chunk each, an uncompressed-DIB tag (01db) on one chunk, ONE ZERO-LENGTH chunk behind
    frame 1 (so frame 2 repeats frame 1), a second RIFF 'AVIX' holding the later frames, an 'ix01' chunk, and no idx1.
    -> (file bytes, the frames a reader must return)."""
    assert len(frames) >= 5
    half = len(frames) // 2
    vid = lambda i, f: chunk(b"01db" if i == 3 else b"01dc", f)
    rec = lambda i, f: riff_list(b"rec ", chunk(b"00wb", b"\x80" * 37) + vid(i, f))
    first = b"".join(rec(i, f) + (chunk(b"01dc", b"") if i == 1 else b"") for i, f in enumerate(frames[:half]))
    movi1 = riff_list(b"movi", chunk(b"ix01", b"\0" * 24) + chunk(b"JUNK", b"j" * 11) + first)
    movi2 = riff_list(b"movi", b"".join(vid(i, f) for i, f in enumerate(frames[half:], half)))
    data = chunk(b"RIFF", b"AVI " + headers(width, height, len(frames) + 1, audio_first=True) + chunk(b"JUNK", b"\0" * 123) + movi1) \
        + chunk(b"RIFF", b"AVIX" + chunk(b"JUNK", b"") + movi2)
    expected = list(frames[:2]) + [frames[1]] + list(frames[2:])
    return data, expected


def pillow_jpeg(px, quality=90, subsampling="4:2:0", restart_rows=0):
    b = io.BytesIO()
    kw = dict(restart_marker_rows=restart_rows) if restart_rows else {}
    Image.fromarray(px).save(b, "JPEG", quality=quality, subsampling=SAMPLING[subsampling], optimize=False, **kw)
    return b.getvalue()


def segments(data):
    """[(marker, offset, total bytes)] of a JPEG file's marker segments from behind SOI up to and including SOS."""
    pos, out = 2, []
    while True:
        assert data[pos] == 0xFF
        m, size = data[pos + 1], data[pos + 2] << 8 | data[pos + 3]
        out.append((m, pos, 2 + size))
        if m == 0xDA:
            return out
        pos += 2 + size


def dht_bytes(data):
    return b"".join(data[at:at + n] for m, at, n in segments(data) if m == 0xC4)


def strip_dht(data):
    """The same file without its DHT segments: an 'AVI1' abbreviated stream."""
    out, pos = bytearray(data[:2]), 2
    for m, at, n in segments(data):
        if m != 0xC4:
            out += data[at:at + n]
        pos = at + n
    return bytes(out + data[pos:])


def clip_pixels(n=12, H=48, W=100, seed=3):
    """n smooth frames with a moving edge and a little noise, u8[n,H,W,3]."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    out = []
    for i in range(n):
        base = np.stack([(xx * 2 + 9 * i) % 256, (yy * 5 + 3 * i) % 256, ((xx + yy) * 2) % 256], -1).astype(np.int32)
        base[:, (7 * i) % W:] = 255 - base[:, (7 * i) % W:]
        out.append(np.clip(base + rng.integers(-6, 7, base.shape), 0, 255).astype(np.uint8))
    return np.stack(out)


def clip_frames(px):
    """Pillow-written files of clip_pixels: 4:2:0 and 4:2:2, with and without restart markers, in turn."""
    kinds = (("4:2:0", 0), ("4:2:2", 0), ("4:2:0", 1), ("4:2:2", 1))
    return [pillow_jpeg(p, 90, *kinds[i % 4]) for i, p in enumerate(px)]
