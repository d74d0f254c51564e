"""A pure-Python model of include/poserisk_hip.h, section j4: the chunk walk of csrc/png_host.cc, inflate by the stated rules
(RFC 1951 with zlib 1.2.11's acceptance rules), the Adler-32, the five filters and the colour rule.  Slow and plain on purpose:
it is what tests/test_png_cpu.py holds against zlib and Pillow, and what the native and GPU tests hold the library against.
`inflate` also reports what it saw (block types, match lengths and distances, code lengths), which tests/png_cases.py uses
to assert its own coverage."""
import struct
import zlib

import numpy as np

ST_REFUSED, ST_TRUNCATED, ST_BAD_CODE, ST_SIZE, ST_FILTER, ST_CHECKSUM = 1, 2, 4, 8, 16, 32
(E_OK, E_SIGNATURE, E_TRUNCATED, E_CRC, E_CHUNK_ORDER, E_DEPTH16, E_DEPTH_SUB8, E_INTERLACE, E_CGBI, E_IHDR, E_SIZE_DIFFERS,
 E_ZLIB_HEADER) = range(12)
SIGNATURE = b"\x89PNG\r\n\x1a\n"
MAX_SIDE = 4096
BPP = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}
LIT_ROOT, DIST_ROOT = 10, 9

LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193,
             12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]


def parse(blob, H=0, W=0):
    """The chunk walk -> dict(status=E_*, and for E_OK width, height, color_type, bpp, idat=[(begin, end)], palette (768 bytes or
    None), zlib_bytes)."""
    blob = bytes(blob)
    if blob[:8] != SIGNATURE:
        return dict(status=E_SIGNATURE)
    p, n = 8, len(blob)
    fr = dict(status=E_OK, idat=[], palette=None)
    have_plte = in_idat = idat_done = False
    while True:
        if n - p < 12:
            return dict(status=E_TRUNCATED)
        ln, = struct.unpack(">I", blob[p:p + 4])
        if ln > n - p - 12:
            return dict(status=E_TRUNCATED)
        typ, body = blob[p + 4:p + 8], blob[p + 8:p + 8 + ln]
        first = p == 8
        if first and typ == b"CgBI":
            return dict(status=E_CGBI)
        if zlib.crc32(typ + body) != struct.unpack(">I", blob[p + 8 + ln:p + 12 + ln])[0]:
            return dict(status=E_CRC)
        if in_idat and typ != b"IDAT":
            in_idat, idat_done = False, True
        if typ == b"IHDR":
            if not first or ln != 13:
                return dict(status=E_CHUNK_ORDER)
            w, h, depth, ct, comp, filt, lace = struct.unpack(">IIBBBBB", body)
            if ct not in BPP:
                return dict(status=E_IHDR)
            if depth == 16:
                return dict(status=E_IHDR if ct == 3 else E_DEPTH16)
            if depth in (1, 2, 4):
                return dict(status=E_DEPTH_SUB8 if ct in (0, 3) else E_IHDR)
            if depth != 8 or comp or filt:
                return dict(status=E_IHDR)
            if lace == 1:
                return dict(status=E_INTERLACE)
            if lace or not (1 <= w <= MAX_SIDE and 1 <= h <= MAX_SIDE):
                return dict(status=E_IHDR)
            fr.update(width=w, height=h, color_type=ct, bpp=BPP[ct])
        elif first:
            return dict(status=E_CHUNK_ORDER)
        elif typ == b"PLTE":
            if have_plte or in_idat or idat_done or ln == 0 or ln > 768 or ln % 3 or fr["color_type"] in (0, 4):
                return dict(status=E_CHUNK_ORDER)
            have_plte = True
            if fr["color_type"] == 3:
                fr["palette"] = body + bytes(768 - ln)
        elif typ == b"IDAT":
            if idat_done or (fr["color_type"] == 3 and not have_plte):
                return dict(status=E_CHUNK_ORDER)
            in_idat = True
            fr["idat"].append((p + 8, p + 8 + ln))
        elif typ == b"IEND":
            if ln:
                return dict(status=E_CHUNK_ORDER)
            break
        p += 12 + ln
    if not fr["idat"]:
        return dict(status=E_CHUNK_ORDER)
    z = b"".join(blob[b:e] for b, e in fr["idat"])
    if len(z) < 2 or z[0] & 15 != 8 or z[0] >> 4 > 7 or z[1] & 32 or (z[0] * 256 + z[1]) % 31:
        return dict(status=E_ZLIB_HEADER)
    fr["zlib_bytes"] = len(z)
    if (H or W) and (fr["height"], fr["width"]) != (H, W):
        return dict(status=E_SIZE_DIFFERS)
    return fr


class _Stop(Exception):
    def __init__(self, status):
        self.status = status


class _Bits:
    def __init__(self, z, at):
        self.v, self.pos, self.end = int.from_bytes(z, "little"), at * 8, len(z) * 8

    def take(self, n):
        if self.pos + n > self.end:
            raise _Stop(ST_TRUNCATED)
        v = (self.v >> self.pos) & ((1 << n) - 1)
        self.pos += n
        return v


def _build(lens, kind):
    """zlib's inflate_table rules -> (count per length, symbols in canonical order); kind 'codes' | 'lens' | 'dists'."""
    cnt = [0] * 16
    for ln in lens:
        cnt[ln] += 1
    cnt[0] = 0
    left, mx = 1, 0
    for ln in range(1, 16):
        left = left * 2 - cnt[ln]
        if left < 0:
            raise _Stop(ST_BAD_CODE)
        if cnt[ln]:
            mx = ln
    if mx == 0:
        if kind != "dists":
            raise _Stop(ST_BAD_CODE)
    elif left > 0 and (kind == "codes" or mx != 1):
        raise _Stop(ST_BAD_CODE)
    return cnt, [s for ln in range(1, 16) for s, x in enumerate(lens) if x == ln]


def _decode(bits, tab):
    cnt, sym = tab
    code = first = index = 0
    for ln in range(1, 16):
        code |= bits.take(1)
        if code - cnt[ln] < first:
            return sym[index + code - first], ln
        index += cnt[ln]
        first = (first + cnt[ln]) << 1
        code <<= 1
    raise _Stop(ST_BAD_CODE)


_FIXED = None


def inflate(z, raw=None):
    """-> (status, output bytes, trailer Adler-32 or None, info).  `raw`: the size the output must have (None: any); output
    that would pass it ends the decode with ST_SIZE.  info: blocks (types in order), matches [(length, distance)], long_codes
    (codes longer than the first-level tables), dyn (per dynamic block: distance codes defined, matches in the block)."""
    global _FIXED
    if _FIXED is None:
        _FIXED = (_build([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8, "lens"), _build([5] * 32, "dists"))
    z = bytes(z)
    out = bytearray()
    info = dict(blocks=[], matches=[], long_codes=0, dyn=[])
    limit = raw if raw is not None else 1 << 62
    try:
        if len(z) < 2:
            raise _Stop(ST_TRUNCATED)
        b = _Bits(z, 2)
        while True:
            final, typ = b.take(1), b.take(2)
            if typ == 3:
                raise _Stop(ST_BAD_CODE)
            info["blocks"].append(typ)
            if typ == 0:
                b.pos = (b.pos + 7) & ~7
                ln, nln = b.take(16), b.take(16)
                if ln != nln ^ 0xFFFF:
                    raise _Stop(ST_BAD_CODE)
                at = b.pos >> 3
                if at + ln > len(z):
                    raise _Stop(ST_TRUNCATED)
                if len(out) + ln > limit:
                    raise _Stop(ST_SIZE)
                out += z[at:at + ln]
                b.pos += 8 * ln
            else:
                if typ == 1:
                    lit, dst = _FIXED
                else:
                    hlit, hdist, hclen = b.take(5) + 257, b.take(5) + 1, b.take(4) + 4
                    if hlit > 286 or hdist > 30:
                        raise _Stop(ST_BAD_CODE)
                    cl = [0] * 19
                    for i in range(hclen):
                        cl[CL_ORDER[i]] = b.take(3)
                    ctab = _build(cl, "codes")
                    lens = []
                    while len(lens) < hlit + hdist:
                        s, _ = _decode(b, ctab)
                        if s < 16:
                            lens.append(s)
                            continue
                        if s == 16:
                            if not lens:
                                raise _Stop(ST_BAD_CODE)
                            rep, val = 3 + b.take(2), lens[-1]
                        elif s == 17:
                            rep, val = 3 + b.take(3), 0
                        else:
                            rep, val = 11 + b.take(7), 0
                        if len(lens) + rep > hlit + hdist:
                            raise _Stop(ST_BAD_CODE)
                        lens += [val] * rep
                    if lens[256] == 0:
                        raise _Stop(ST_BAD_CODE)
                    lit, dst = _build(lens[:hlit], "lens"), _build(lens[hlit:], "dists")
                    info["dyn"].append([sum(1 for x in lens[hlit:] if x), 0])
                while True:
                    s, cl_len = _decode(b, lit)
                    info["long_codes"] += cl_len > LIT_ROOT
                    if s < 256:
                        if len(out) >= limit:
                            raise _Stop(ST_SIZE)
                        out.append(s)
                        continue
                    if s == 256:
                        break
                    if s > 285:
                        raise _Stop(ST_BAD_CODE)
                    length = LEN_BASE[s - 257] + b.take(LEN_EXTRA[s - 257])
                    d, cl_len = _decode(b, dst)
                    info["long_codes"] += cl_len > DIST_ROOT
                    if d > 29:
                        raise _Stop(ST_BAD_CODE)
                    dist = DIST_BASE[d] + b.take(DIST_EXTRA[d])
                    if dist > len(out):
                        raise _Stop(ST_BAD_CODE)
                    if len(out) + length > limit:
                        raise _Stop(ST_SIZE)
                    info["matches"].append((length, dist))
                    if typ == 2:
                        info["dyn"][-1][1] += 1
                    if dist >= length:
                        out += out[len(out) - dist:len(out) - dist + length]
                    else:
                        period = bytes(out[-dist:])
                        out += (period * (length // dist + 1))[:length]
            if final:
                break
        b.pos = (b.pos + 7) & ~7
        adler = b.take(8) << 24 | b.take(8) << 16 | b.take(8) << 8 | b.take(8)
    except _Stop as e:
        return e.status, bytes(out), None, info
    if raw is not None and len(out) != raw:
        return ST_SIZE, bytes(out), adler, info
    return 0, bytes(out), adler, info


def adler32(data):
    a, b = 1, 0
    for x in data:
        a = (a + x) % 65521
        b = (b + a) % 65521
    return b << 16 | a


def _paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    return a if pa <= pb and pa <= pc else b if pb <= pc else c


def unfilter(raw, H, W, bpp):
    """-> (status 0 | ST_FILTER, u8[H, W * bpp] unfiltered bytes); a filter byte above 4 is taken as 0."""
    stride, status = 1 + W * bpp, 0
    rows = np.frombuffer(raw, np.uint8).reshape(H, stride)
    out = np.zeros((H, W * bpp), np.int64)
    prev = [0] * (W * bpp)
    for y in range(H):
        ft, x = int(rows[y, 0]), rows[y, 1:].tolist()
        if ft > 4:
            ft, status = 0, ST_FILTER
        if ft == 1:
            for i in range(bpp, len(x)):
                x[i] = (x[i] + x[i - bpp]) & 255
        elif ft == 2:
            x = [(v + u) & 255 for v, u in zip(x, prev)]
        elif ft == 3:
            for i in range(len(x)):
                x[i] = (x[i] + (((x[i - bpp] if i >= bpp else 0) + prev[i]) >> 1)) & 255
        elif ft == 4:
            for i in range(len(x)):
                a, c = (x[i - bpp], prev[i - bpp]) if i >= bpp else (0, 0)
                x[i] = (x[i] + _paeth(a, prev[i], c)) & 255
        out[y] = prev = x
    return status, out.astype(np.uint8)


def colour(px, fr, bgr=False):
    """u8[H, W * bpp] unfiltered bytes -> u8[H, W, 3]."""
    H, W, ct = fr["height"], fr["width"], fr["color_type"]
    px = px.reshape(H, W, fr["bpp"])
    if ct == 3:
        rgb = np.frombuffer(fr["palette"], np.uint8).reshape(256, 3)[px[..., 0]]
    elif ct in (2, 6):
        rgb = px[..., :3]
    else:
        rgb = np.repeat(px[..., :1], 3, axis=2)
    return np.ascontiguousarray(rgb[..., ::-1] if bgr else rgb)


def decode(blob, bgr=False, H=0, W=0, want_info=False):
    """The whole contract on one file -> (parse status, device status, u8[H, W, 3] pixels or None for a refused file)."""
    fr = parse(blob, H, W)
    if fr["status"]:
        return (fr["status"], ST_REFUSED, None) + ((None,) if want_info else ())
    z = b"".join(bytes(blob[b:e]) for b, e in fr["idat"])
    h, w, bpp = fr["height"], fr["width"], fr["bpp"]
    nraw = h * (1 + w * bpp)
    st, raw, adler, info = inflate(z, nraw)
    if st:
        px = np.zeros((h, w, 3), np.uint8)
    else:
        if adler32(raw) != adler:
            st |= ST_CHECKSUM
        fst, un = unfilter(raw, h, w, bpp)
        st |= fst
        px = colour(un, fr, bgr)
    return (E_OK, st, px) + ((info,) if want_info else ())


def zlib_verdict(z, nraw):
    """What zlib itself says of a stream that must inflate to nraw bytes: the bytes, or None where zlib.decompress raises or
    the length differs."""
    try:
        out = zlib.decompress(z)
    except zlib.error:
        return None
    return out if len(out) == nraw else None
