"""A small RIFF AVI reader for the tests, written from the container's definition and independent of
poserisk_release_amd/mjpeg.py: it walks chunks by their own sizes and trusts nothing else."""
import struct


def _chunks(data, lo, hi):
    """(fourcc, payload offset, size) of the chunks in data[lo:hi]; a chunk is padded to an even length."""
    while lo + 8 <= hi:
        tag, size = data[lo:lo + 4], struct.unpack_from("<I", data, lo + 4)[0]
        assert lo + 8 + size <= hi, f"chunk {tag!r} at {lo} leaves its parent"
        yield tag, lo + 8, size
        lo += 8 + size + (size & 1)
    assert lo == hi, f"{hi - lo} stray bytes behind the last chunk"


def read_avi(path):
    """-> dict(width, height, fps, count (avih), stream_count (strh), handler, compression, frames [bytes], index [(offset, size)],
    odd_padded: every odd-length frame is followed by a zero pad byte)."""
    data = open(path, "rb").read()
    assert data[:4] == b"RIFF" and data[8:12] == b"AVI " and struct.unpack_from("<I", data, 4)[0] == len(data) - 8
    out = dict(frames=[], index=[], odd_padded=True)
    movi_tag = None
    for tag, lo, size in _chunks(data, 12, len(data)):
        if tag == b"LIST" and data[lo:lo + 4] == b"hdrl":
            for t, a, n in _chunks(data, lo + 4, lo + size):
                if t == b"avih":
                    usec, _, _, flags, count, _, streams, _, w, h = struct.unpack_from("<10I", data, a)
                    out.update(usec_per_frame=usec, count=count, width=w, height=h, has_index=bool(flags & 0x10), streams=streams)
                elif t == b"LIST" and data[a:a + 4] == b"strl":
                    for t2, a2, n2 in _chunks(data, a + 4, a + n):
                        if t2 == b"strh":
                            out["type"], out["handler"] = data[a2:a2 + 4], data[a2 + 4:a2 + 8]
                            scale, rate, _, length = struct.unpack_from("<4I", data, a2 + 20)
                            out.update(fps=rate / scale, stream_count=length)
                        elif t2 == b"strf":
                            bi = struct.unpack_from("<IiiHH4s", data, a2)
                            out.update(bi_width=bi[1], bi_height=bi[2], compression=bi[5])
        elif tag == b"LIST" and data[lo:lo + 4] == b"movi":
            movi_tag = lo
            for t, a, n in _chunks(data, lo + 4, lo + size):
                assert t == b"00dc", t
                out["frames"].append(data[a:a + n])
                out.setdefault("offsets", []).append(a - 8 - movi_tag)
                if n & 1 and data[a + n:a + n + 1] != b"\0":
                    out["odd_padded"] = False
        elif tag == b"idx1":
            for i in range(size // 16):
                ckid, flags, off, n = struct.unpack_from("<4sIII", data, lo + 16 * i)
                assert ckid == b"00dc" and flags & 0x10
                out["index"].append((off, n))
    return out
