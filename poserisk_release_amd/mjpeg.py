"""Motion-JPEG in a RIFF AVI 1.0 container, written in pure Python: the file behind `<TITLE>_video.avi` and `<TITLE>_mesh.avi`
when the frames were encoded on the GPU (jpeg.encode_frames; the gpu_video_codec knob of dropin/core/base.py).  Every frame is
one complete baseline JPEG file, stored as it is: nothing here looks inside it.

    RIFF 'AVI '
      LIST 'hdrl'   avih (main header)   LIST 'strl'   strh ('vids' / 'MJPG')   strf (BITMAPINFOHEADER)
      LIST 'movi'   '00dc' chunks, one per frame, padded to an even length
      idx1          one entry per frame: '00dc', key frame, offset from the 'movi' tag, length

Frame counts and sizes are patched into the headers on close().  One RIFF cannot index past 32-bit offsets, so at `split_bytes`
the file is closed and the frames continue in `<name>.001.avi`, `<name>.002.avi`, ...: `paths` lists what was written.

`AviReader` is the other direction, for any Motion-JPEG AVI (a camera's, `ffmpeg -c:v mjpeg`'s, AviWriter's): it walks the RIFF
chunks trusting only their sizes, never the index, and returns the video stream's chunks, each one complete JPEG file.  The one
thing it does to a frame: a frame without Huffman tables (the "AVI1" abbreviated streams many cameras write) gets the standard
tables, `STD_DHT`, spliced in front of its SOS, so that the decoder, which refuses a stream without tables, can read it."""
import mmap
import os
import re
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


# ITU T.81 Annex K.3, the tables libjpeg assumes for a stream that brings none, as the four DHT segments (DC 0, AC 0, DC 1,
# AC 1) that libjpeg writes and pr_jpeg_encode_plan puts into its header: 2 * (33 + 183) = 432 bytes.  (As ONE segment, the form
# ffmpeg's mjpeg2jpeg filter splices, the same tables take 420 bytes.)  tests/test_frontend_cpu.py holds them against both.
STD_DHT = bytes.fromhex(
    "ffc4001f0000010501010101010100000000000000000102030405060708090a0bffc400b5100002010303020403050504040000017d010203000411"
    "05122131410613516107227114328191a1082342b1c11552d1f02433627282090a161718191a25262728292a3435363738393a434445464748494a53"
    "5455565758595a636465666768696a737475767778797a838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3"
    "c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae1e2e3e4e5e6e7e8e9eaf1f2f3f4f5f6f7f8f9faffc4001f0100030101010101010101010000000000000102"
    "030405060708090a0bffc400b51100020102040403040705040400010277000102031104052131061241510761711322328108144291a1b1c1092333"
    "52f0156272d10a162434e125f11718191a262728292a35363738393a434445464748494a535455565758595a636465666768696a737475767778797a"
    "82838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae2e3e4e5e6e7"
    "e8e9eaf2f3f4f5f6f7f8f9fa")
_FRAME_LISTS = (b"movi", b"rec ")
_NEXT_MARKER = re.compile(rb"\xff[^\x00\xd0-\xd7\xff]")   # inside entropy-coded data: the first marker that is not stuffing or RSTn


def is_avi(path):
    """Does the file start as a RIFF AVI does?  (Nothing else is looked at: AviReader says whether it can be read.)"""
    try:
        with open(path, "rb") as f:
            head = f.read(12)
    except OSError:
        return False
    return len(head) == 12 and head[:4] == b"RIFF" and head[8:12] == b"AVI "


def inspect_frame(data):
    """Walk the marker segments of one JPEG file up to its SOS -> (offset of the SOS marker or -1 when the walk does not reach
    one, whether a DHT segment came before it, the field polarity of an 'AVI1' APP0 segment or 0, whether a second SOI follows
    the frame's EOI).  Segments are stepped over by their lengths: bytes inside an APPn segment (an EXIF thumbnail is a whole
    JPEG file) are never taken for markers."""
    n, pos, has_dht, polarity = len(data), 2, False, 0
    if n < 4 or data[0] != 0xFF or data[1] != 0xD8:
        return -1, False, 0, False
    while pos + 4 <= n:
        if data[pos] != 0xFF:
            return -1, has_dht, polarity, False
        m = data[pos + 1]
        if m == 0xFF:                                      # a fill byte
            pos += 1
            continue
        if m == 0x01 or 0xD0 <= m <= 0xD7:                 # markers without a length
            pos += 2
            continue
        if m == 0xD9 or m == 0xD8:
            return -1, has_dht, polarity, False
        size = data[pos + 2] << 8 | data[pos + 3]
        if size < 2 or pos + 2 + size > n:
            return -1, has_dht, polarity, False
        if m == 0xDA:
            nxt = _NEXT_MARKER.search(data, pos + 2 + size)
            second = False
            if nxt is not None and data[nxt.start() + 1] == 0xD9:
                rest = bytes(data[nxt.start() + 2:nxt.start() + 2 + 64]).lstrip(b"\x00")
                while rest[:2] == b"\xff\xff":
                    rest = rest[1:]
                second = rest[:2] == b"\xff\xd8"
            return pos, has_dht, polarity, second
        if m == 0xC4:
            has_dht = True
        elif m == 0xE0 and size >= 7 and bytes(data[pos + 4:pos + 8]) == b"AVI1":
            polarity = data[pos + 8]
        pos += 2 + size
    return -1, has_dht, polarity, False


class AviReader:
    """The first video stream of a Motion-JPEG AVI file: `.fps`, `.n_frames`, `.header` (what avih, strh and strf say:
    informational, the size that counts is each JPEG's own), `.paths` (the file and its continuation files) and `.frames()`.

    Walks `RIFF 'AVI '` and every following `RIFF 'AVIX'` (OpenDML), descends into `LIST 'movi'` and `LIST 'rec '`, takes
    every `##dc` / `##db` chunk of the first 'vids' stream in file order and skips everything else (JUNK, idx1, ix##, indx,
    audio).  Only chunk sizes are trusted: a chunk that does not fit its parent (a truncated file) is refused, the index is
    neither needed nor read.  A zero-length chunk repeats the previous frame, as players do.  `<stem>.001<ext>`, ... beside
    the named file (what AviWriter writes at split_bytes) are read as its continuation.  Raises ValueError, naming the file and
    the reason, for anything that is not progressive-scan Motion-JPEG: another codec (the fourcc is named), no video stream, no
    RIFF, interlaced Motion-JPEG (two fields in a chunk, or an AVI1 segment with field polarity 1 or 2)."""

    def __init__(self, path):
        self.path = str(path)
        self.paths, self.header, self._frames = [], None, []
        stem, ext = os.path.splitext(self.path)
        k = 0
        while True:
            p = self.path if k == 0 else f"{stem}.{k:03d}{ext}"
            if k and not os.path.isfile(p):
                break
            header = self._read_file(p)
            if k == 0:
                self.header = header
            self.paths.append(p)
            k += 1
        h = self.header
        if h["rate"] and h["scale"]:
            self.fps = h["rate"] / h["scale"]
        elif h["us_per_frame"]:
            self.fps = 1e6 / h["us_per_frame"]
        else:
            self.fps = 30.0
        self.n_frames = len(self._frames)

    def frames(self):
        """[bytes], one complete JPEG file per frame (with STD_DHT spliced in where the stream brought no tables)."""
        return list(self._frames)

    # ---- one file ---------------------------------------------------------------------------------------------------------
    def _read_file(self, path):
        def bad(why):
            return ValueError(f"{path!r}: {why}")
        size = os.path.getsize(path)
        if size < 12:
            raise bad(f"not a RIFF AVI file ({size} bytes)")
        with open(path, "rb") as f, mmap.mmap(f.fileno(), 0, access=mmap.ACCESS_READ) as data:
            if data[:4] != b"RIFF" or data[8:12] != b"AVI ":
                raise bad(f"not a RIFF AVI file (it starts with {bytes(data[:4])!r} ... {bytes(data[8:12])!r})")
            header = dict(us_per_frame=0, total_frames=0, width=0, height=0, streams=0, handler=b"", compression=b"", rate=0,
                          scale=0, length=0, strf_width=0, strf_height=0, video_stream=-1)
            state = dict(streams=0, first=len(self._frames))

            def chunks(lo, hi, parent):
                pos = lo
                while pos + 8 <= hi:
                    tag = bytes(data[pos:pos + 4])
                    n = struct.unpack_from("<I", data, pos + 4)[0]
                    if n > hi - (pos + 8):
                        raise bad(f"chunk {tag!r} at offset {pos} ({n} bytes) leaves its parent {parent} which ends at {hi}: "
                                  "the file is truncated or damaged")
                    yield tag, pos + 8, n
                    pos += 8 + n + (n & 1)

            def video_chunk(tag):
                v = header["video_stream"]
                return v >= 0 and tag[2:4] in (b"dc", b"db") and tag[:2] == b"%02d" % v

            def walk_movi(lo, hi, parent):
                for tag, at, n in chunks(lo, hi, parent):
                    if tag == b"LIST":
                        if n >= 4 and bytes(data[at:at + 4]) in _FRAME_LISTS:
                            walk_movi(at + 4, at + n, f"LIST {bytes(data[at:at + 4])!r}")
                    elif video_chunk(tag):
                        self._take(path, bytes(data[at:at + n]), state["first"])

            def walk_strl(lo, hi):
                fcc_type = None
                for tag, at, n in chunks(lo, hi, "LIST b'strl'"):
                    if tag == b"strh" and n >= 36:
                        fcc_type = bytes(data[at:at + 4])
                        if fcc_type == b"vids" and header["video_stream"] < 0:
                            header["video_stream"] = state["streams"]
                            header["handler"] = bytes(data[at + 4:at + 8])
                            header["scale"], header["rate"] = struct.unpack_from("<II", data, at + 20)
                            header["length"] = struct.unpack_from("<I", data, at + 32)[0]
                        else:
                            fcc_type = None
                    elif tag == b"strf" and fcc_type == b"vids" and n >= 20:
                        header["strf_width"], header["strf_height"] = struct.unpack_from("<ii", data, at + 4)
                        header["compression"] = bytes(data[at + 16:at + 20])
                        fcc_type = None
                state["streams"] += 1

            def walk_hdrl(lo, hi):
                for tag, at, n in chunks(lo, hi, "LIST b'hdrl'"):
                    if tag == b"avih" and n >= 40:
                        v = struct.unpack_from("<10I", data, at)
                        header.update(us_per_frame=v[0], total_frames=v[4], streams=v[6], width=v[8], height=v[9])
                    elif tag == b"LIST" and n >= 4 and bytes(data[at:at + 4]) == b"strl":
                        walk_strl(at + 4, at + n)

            checked = False
            for tag, at, n in chunks(0, size, "the file"):
                if tag != b"RIFF":
                    break                                      # bytes behind the last RIFF chunk are nobody's
                form = bytes(data[at:at + 4]) if n >= 4 else b""
                if form not in (b"AVI ", b"AVIX"):
                    continue
                for tag2, at2, n2 in chunks(at + 4, at + n, f"RIFF {form!r}"):
                    if tag2 != b"LIST" or n2 < 4:
                        continue
                    kind = bytes(data[at2:at2 + 4])
                    if kind == b"hdrl" and form == b"AVI ":
                        walk_hdrl(at2 + 4, at2 + n2)
                    elif kind == b"movi":
                        if not checked:
                            self._check_codec(header, bad)
                            checked = True
                        walk_movi(at2 + 4, at2 + n2, "LIST b'movi'")
            if not checked:
                self._check_codec(header, bad)
        return header

    @staticmethod
    def _check_codec(header, bad):
        if header["video_stream"] < 0:
            raise bad("no video stream (no 'strl' list whose 'strh' says 'vids')")
        if b"mjpg" not in (header["handler"].lower(), header["compression"].lower()):
            raise bad(f"the video stream is {header['compression']!r} (stream handler {header['handler']!r}), not Motion-JPEG "
                      "(MJPG): only Motion-JPEG video is read here")

    def _take(self, path, data, first):
        index = len(self._frames)
        where = f"{path!r}: frame {index - first}"
        if not data:
            if index == first:
                raise ValueError(f"{where}: the first video chunk is empty (an empty chunk repeats the previous frame, and "
                                 "there is none)")
            self._frames.append(self._frames[-1])
            return
        sos, has_dht, polarity, second_soi = inspect_frame(data)
        if polarity in (1, 2) or second_soi:
            raise ValueError(f"{where}: interlaced Motion-JPEG ("
                             + (f"AVI1 field polarity {polarity}" if polarity in (1, 2) else "two SOI markers: two fields in one chunk")
                             + ") is not supported")
        if sos >= 0 and not has_dht:
            data = data[:sos] + STD_DHT + data[sos:]
        self._frames.append(data)
