"""Motion-JPEG in a RIFF AVI 1.0 container, written in pure Python: the file behind `<TITLE>_video.avi` and `<TITLE>_mesh.avi`
when the frames were encoded on the GPU (jpeg.encode_frames; the gpu_video_codec knob of dropin/core/base.py).  Every frame is
one complete baseline JPEG file, stored as it is: nothing here looks inside it.

    RIFF 'AVI '
      LIST 'hdrl'   avih (main header)   LIST 'strl'   strh ('vids' / 'MJPG')   strf (BITMAPINFOHEADER)
      LIST 'movi'   '00dc' chunks, one per frame, padded to an even length
      idx1          one entry per frame: '00dc', key frame, offset from the 'movi' tag, length

Frame counts and sizes are patched into the headers on close().  One RIFF cannot index past 32-bit offsets, so at `split_bytes`
the file is closed and the frames continue in `<name>.001.avi`, `<name>.002.avi`, ...: `paths` lists what was written."""
import os
import struct
from fractions import Fraction

_AVIF_HASINDEX, _AVIIF_KEYFRAME = 0x10, 0x10
_HEADER_BYTES = 12 + 12 + 8 + 56 + 12 + 8 + 56 + 8 + 40 + 12          # everything in front of the first '00dc'


class AviWriter:
    def __init__(self, path, width, height, fps, split_bytes=1 << 30):
        if not (0 < int(width) < 65536 and 0 < int(height) < 65536):
            raise ValueError(f"AviWriter: {width} x {height} frames")
        if not fps > 0:
            raise ValueError(f"AviWriter: fps = {fps!r}")
        if not 4096 <= int(split_bytes) <= 0xFFFF0000:
            raise ValueError(f"AviWriter: split_bytes = {split_bytes!r} outside 4096..0xFFFF0000 (one RIFF holds 32-bit sizes)")
        self.path, self.width, self.height, self.split_bytes = str(path), int(width), int(height), int(split_bytes)
        rate = Fraction(float(fps)).limit_denominator(100000)
        self.rate, self.scale = rate.numerator, rate.denominator
        self.paths, self.frames_written = [], 0
        self._f = None
        self._open()

    def _open(self):
        stem, ext = os.path.splitext(self.path)
        n = len(self.paths)
        path = self.path if n == 0 else f"{stem}.{n:03d}{ext}"
        self._f = open(path, "wb")
        self.paths.append(path)
        self._index, self._largest, self._pos = [], 0, _HEADER_BYTES
        self._f.write(self._headers(0))

    def _headers(self, movi_bytes):
        n, w, h = len(self._index), self.width, self.height
        per_second = int(self._pos * self.rate / (self.scale * max(n, 1)))
        avih = struct.pack("<14I", round(1e6 * self.scale / self.rate), min(per_second, 0xFFFFFFFF), 0, _AVIF_HASINDEX, n, 0, 1,
                           self._largest, w, h, 0, 0, 0, 0)
        strh = struct.pack("<4s4sIHHIIIIIIiI4H", b"vids", b"MJPG", 0, 0, 0, 0, self.scale, self.rate, 0, n, self._largest, -1, 0,
                           0, 0, w, h)
        strf = struct.pack("<IiiHH4sIiiII", 40, w, h, 1, 24, b"MJPG", w * h * 3, 0, 0, 0, 0)
        strl = b"strl" + b"strh" + struct.pack("<I", len(strh)) + strh + b"strf" + struct.pack("<I", len(strf)) + strf
        hdrl = b"hdrl" + b"avih" + struct.pack("<I", len(avih)) + avih + b"LIST" + struct.pack("<I", len(strl)) + strl
        head = b"LIST" + struct.pack("<I", len(hdrl)) + hdrl + b"LIST" + struct.pack("<I", 4 + movi_bytes) + b"movi"
        riff_bytes = 4 + len(head) + movi_bytes + (8 + 16 * n)
        out = b"RIFF" + struct.pack("<I", riff_bytes) + b"AVI " + head
        assert len(out) == _HEADER_BYTES
        return out

    def write(self, jpeg_bytes):
        """Append one frame: a complete JPEG file as bytes."""
        if self._f is None:
            raise ValueError("AviWriter: write() after close()")
        data = bytes(jpeg_bytes)
        chunk = 8 + len(data) + (len(data) & 1)
        if chunk + _HEADER_BYTES + 24 > self.split_bytes:
            raise ValueError(f"AviWriter: a frame of {len(data)} bytes does not fit a file of split_bytes = {self.split_bytes}")
        if self._index and self._pos + chunk + 8 + 16 * (len(self._index) + 1) > self.split_bytes:
            self._finish()
            self._open()
        self._f.write(b"00dc" + struct.pack("<I", len(data)) + data + (b"\0" if len(data) & 1 else b""))
        self._index.append((self._pos - _HEADER_BYTES + 4, len(data)))       # offset of the chunk from the 'movi' tag
        self._largest = max(self._largest, len(data))
        self._pos += chunk
        self.frames_written += 1

    def _finish(self):
        f, self._f = self._f, None
        f.write(b"idx1" + struct.pack("<I", 16 * len(self._index)))
        f.write(b"".join(b"00dc" + struct.pack("<III", _AVIIF_KEYFRAME, off, size) for off, size in self._index))
        f.seek(0)
        f.write(self._headers(self._pos - _HEADER_BYTES))
        f.close()

    def close(self):
        """Write the index, patch counts and sizes into the headers; returns the list of files written."""
        if self._f is not None:
            self._finish()
        return self.paths

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
