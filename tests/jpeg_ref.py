"""The JPEG contract of include/poserisk_hip.h (section j1: pr_jpeg_parse, pr_jpeg_decode) restated in numpy and plain Python:
marker parsing, Huffman decoding, the islow IDCT in 64-bit, fancy upsampling and the fixed-point colour conversion.  Written
from the contract and from the JPEG standard (ITU-T T.81), not from the kernels: csrc/jpeg_host.cc and csrc/jpeg.hip are checked
against this file, and this file against libjpeg's pixels (tests/golden/jpeg_cases.npz, and Pillow where it is importable).
A reference implementation: slow (the entropy decoder is a Python loop).  On a stream the parser's rules accept but that cannot
be decoded (a code no table holds, a run past coefficient 63, data that ends early, a block outside the 32-bit IDCT bound) it
raises BadStream: those are the conditions for which the device must report a non-zero status."""
import numpy as np

OK, NOT_JPEG, TRUNCATED, PROGRESSIVE, EXTENDED, ARITHMETIC, PRECISION, COMPONENTS, SAMPLING, SCANS, QUANT16, DIMENSIONS, \
    SIZE_DIFFERS, TABLE, MARKER, RESTARTS = range(16)
IDCT_BOUND = 35079

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14,
                   21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53,
                   60, 61, 54, 47, 55, 62, 63])


class Refused(Exception):
    def __init__(self, code):
        super().__init__(f"refusal {code}")
        self.code = code


class BadStream(Exception):
    pass


def _need(cond, code):
    if not cond:
        raise Refused(code)


def parse(data):
    """bytes -> dict(width, height, ncomp, hs, vs, restart, quant u16[ncomp,64] natural order, dc_sel, ac_sel,
    huff {(class, id): (bits[16], vals)} for the tables the scan uses, segments [(begin, end, first_mcu)]); raises Refused."""
    d = bytes(data)
    n = len(d)
    _need(n >= 2 and d[0] == 0xFF and d[1] == 0xD8, NOT_JPEG)
    pos = 2
    qt, huff, sof, restart = {}, {}, None, 0
    while True:
        _need(pos + 2 <= n, TRUNCATED)
        _need(d[pos] == 0xFF, MARKER)
        m = d[pos + 1]
        pos += 2
        while m == 0xFF:
            _need(pos < n, TRUNCATED)
            m = d[pos]
            pos += 1
        _need(m != 0xD9, SCANS)
        _need(not (m in (0, 1) or 0xD0 <= m <= 0xD8), MARKER)
        _need(pos + 2 <= n, TRUNCATED)
        ln = d[pos] << 8 | d[pos + 1]
        _need(ln >= 2, MARKER)
        _need(pos + ln <= n, TRUNCATED)
        seg = d[pos + 2:pos + ln]
        pos += ln
        _need(m != 0xC2, PROGRESSIVE)
        _need(m not in (0xC9, 0xCA, 0xCB, 0xCC, 0xCD, 0xCE, 0xCF), ARITHMETIC)
        _need(m not in (0xC1, 0xC3, 0xC5, 0xC6, 0xC7, 0xC8, 0xDC, 0xDE, 0xDF), EXTENDED)
        if m == 0xC0:
            _need(sof is None and len(seg) >= 6, MARKER)
            prec, h, w, nc = seg[0], seg[1] << 8 | seg[2], seg[3] << 8 | seg[4], seg[5]
            _need(prec == 8, PRECISION)
            _need(nc in (1, 3), COMPONENTS)
            _need(16 <= h <= 4096 and 16 <= w <= 4096, DIMENSIONS)
            _need(len(seg) == 6 + 3 * nc, MARKER)
            comps = []
            for c in range(nc):
                cid, hv, tq = seg[6 + 3 * c:9 + 3 * c]
                _need(1 <= hv >> 4 <= 4 and 1 <= hv & 15 <= 4, SAMPLING)
                _need(tq <= 3, TABLE)
                _need(all(cid != o[0] for o in comps), MARKER)
                comps.append((cid, hv >> 4, hv & 15, tq))
            if nc == 3:
                _need((comps[0][1], comps[0][2]) in ((1, 1), (2, 1), (2, 2)), SAMPLING)
                _need(all(c[1] == 1 and c[2] == 1 for c in comps[1:]), SAMPLING)
            sof = dict(width=w, height=h, ncomp=nc, hs=comps[0][1] if nc == 3 else 1, vs=comps[0][2] if nc == 3 else 1, comps=comps)
        elif m == 0xDB:
            p = 0
            while p < len(seg):
                pq = seg[p]
                _need(pq >> 4 != 1, QUANT16)
                _need(pq >> 4 == 0 and pq & 15 <= 3, TABLE)
                _need(p + 65 <= len(seg), MARKER)
                t = np.zeros(64, np.uint16)
                t[ZIGZAG] = np.frombuffer(seg[p + 1:p + 65], np.uint8)
                qt[pq & 15] = t
                p += 65
        elif m == 0xC4:
            p = 0
            while p < len(seg):
                tc = seg[p]
                _need(tc >> 4 <= 1 and tc & 15 <= 1, TABLE)
                _need(p + 17 <= len(seg), MARKER)
                bits = list(seg[p + 1:p + 17])
                _need(sum(bits) <= 256 and p + 17 + sum(bits) <= len(seg), TABLE)
                vals = list(seg[p + 17:p + 17 + sum(bits)])
                _need(tc >> 4 == 1 or all(v <= 15 for v in vals), TABLE)
                huff[(tc >> 4, tc & 15)] = (bits, vals)
                p += 17 + sum(bits)
        elif m == 0xDD:
            _need(len(seg) == 2, MARKER)
            restart = seg[0] << 8 | seg[1]
        elif m == 0xDA:
            _need(sof is not None and len(seg) >= 1, MARKER)
            ns = seg[0]
            _need(ns == sof["ncomp"], SCANS)
            _need(len(seg) == 1 + 2 * ns + 3, MARKER)
            dc_sel, ac_sel, quant = [], [], []
            for c in range(ns):
                cid, sel = seg[1 + 2 * c], seg[2 + 2 * c]
                _need(cid == sof["comps"][c][0], SCANS)
                _need(sel >> 4 <= 1 and sel & 15 <= 1, TABLE)
                _need((0, sel >> 4) in huff and (1, sel & 15) in huff and sof["comps"][c][3] in qt, TABLE)
                dc_sel.append(sel >> 4)
                ac_sel.append(sel & 15)
                quant.append(qt[sof["comps"][c][3]])
            _need(tuple(seg[1 + 2 * ns:]) == (0, 63, 0), PROGRESSIVE)
            break
    out = dict(sof, restart=restart, quant=np.stack(quant), dc_sel=dc_sel, ac_sel=ac_sel)
    del out["comps"]
    out["huff"] = {k: huff[k] for k in {(0, s) for s in dc_sel} | {(1, s) for s in ac_sel}}
    for bits, _ in out["huff"].values():            # the counts must form a prefix code
        code = 0
        for l in range(16):
            _need(code + bits[l] <= 1 << (l + 1), TABLE)
            code = (code + bits[l]) << 1
    mcus = -(-sof["width"] // (8 * out["hs"])) * -(-sof["height"] // (8 * out["vs"]))
    want = -(-mcus // restart) if restart else 1
    segs, begin, closing = [], pos, None
    while pos < n:
        pos = d.find(b"\xff", pos)
        if pos < 0 or pos + 1 >= n:
            break
        m = d[pos + 1]
        if m == 0:
            pos += 2
        elif m == 0xFF:
            pos += 1
        else:
            _need(len(segs) < want, RESTARTS)
            segs.append((begin, pos, len(segs) * restart))
            if 0xD0 <= m <= 0xD7:
                _need(restart and m == 0xD0 + (len(segs) - 1) % 8, RESTARTS)
                pos += 2
                begin = pos
                continue
            closing = m
            break
    _need(closing is not None, TRUNCATED)
    _need(closing not in (0xDA, 0xC4, 0xDB, 0xDD), SCANS)
    _need(closing == 0xD9, MARKER)
    _need(len(segs) == want, RESTARTS)
    out["segments"] = segs
    return out


def parse_status(data):
    try:
        parse(data)
        return OK
    except Refused as e:
        return e.code


def _codes(bits, vals):
    table, code, k = {}, 0, 0
    for l in range(1, 17):
        for _ in range(bits[l - 1]):
            table[(l, code)] = vals[k]
            code += 1
            k += 1
        code <<= 1
    return table


class _Bits:
    def __init__(self, d):                        # d: the segment with stuffing removed
        self.d, self.pos = d, 0

    def bit(self):
        byte = self.d[self.pos >> 3] if (self.pos >> 3) < len(self.d) else 0
        self.pos += 1
        return (byte >> (7 - ((self.pos - 1) & 7))) & 1

    def symbol(self, table):
        code = 0
        for l in range(1, 17):
            code = code << 1 | self.bit()
            if (l, code) in table:
                return table[(l, code)]
        raise BadStream("a code no table holds")

    def extend(self, s):
        r = 0
        for _ in range(s):
            r = r << 1 | self.bit()
        return r if r >= 1 << (s - 1) else r - (1 << s) + 1


def geometry(p):
    mx, my = -(-p["width"] // (8 * p["hs"])), -(-p["height"] // (8 * p["vs"]))
    return mx, my, [(mx * p["hs"], my * p["vs"])] + [(mx, my)] * (p["ncomp"] - 1)


def coefficients(data, p=None):
    """Quantised coefficients per component: list of int32[bh, bw, 64] in natural order."""
    d = bytes(data)
    p = p or parse(d)
    mx, my, blocks = geometry(p)
    coef = [np.zeros((bh, bw, 64), np.int32) for bw, bh in blocks]
    tabs = {k: _codes(*v) for k, v in p["huff"].items()}
    for begin, end, first in p["segments"]:
        raw = d[begin:end]
        cut = raw.find(b"\xff\xff")
        raw = raw if cut < 0 else raw[:cut]
        b = _Bits(raw.replace(b"\xff\x00", b"\xff"))
        pred = [0] * p["ncomp"]
        n = min(p["restart"], mx * my - first) if p["restart"] else mx * my
        for mcu in range(first, first + n):
            for c in range(p["ncomp"]):
                hc, vc = (p["hs"], p["vs"]) if c == 0 else (1, 1)
                for blk in range(hc * vc):
                    out = coef[c][(mcu // mx) * vc + blk // hc, (mcu % mx) * hc + blk % hc]
                    s = b.symbol(tabs[(0, p["dc_sel"][c])])
                    if s:
                        pred[c] += b.extend(s)
                    if not -32768 <= pred[c] <= 32767:
                        raise BadStream("a DC value outside int16")
                    out[0] = pred[c]
                    k = 1
                    while k < 64:
                        rs = b.symbol(tabs[(1, p["ac_sel"][c])])
                        r, s = rs >> 4, rs & 15
                        if s == 0:
                            if r != 15:
                                break
                            k += 16
                            if k > 63:
                                raise BadStream("sixteen zeros with no coefficient left behind them")
                            continue
                        k += r
                        if k > 63:
                            raise BadStream("a run past coefficient 63")
                        out[ZIGZAG[k]] = b.extend(s)
                        k += 1
        if b.pos > 8 * len(b.d):
            raise BadStream("the segment's data ends early")
    return coef


def _pass(i, shift):
    i0, i1, i2, i3, i4, i5, i6, i7 = i
    z1 = (i2 + i6) * 4433
    t2 = z1 - i6 * 15137
    t3 = z1 + i2 * 6270
    t0 = (i0 + i4) << 13
    t1 = (i0 - i4) << 13
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    a0, a1, a2, a3 = i7, i5, i3, i1
    z1, z2, z3, z4 = a0 + a3, a1 + a2, a0 + a2, a1 + a3
    z5 = (z3 + z4) * 9633
    a0, a1, a2, a3 = a0 * 2446, a1 * 16819, a2 * 25172, a3 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    a0, a1, a2, a3 = a0 + z1 + z3, a1 + z2 + z4, a2 + z2 + z3, a3 + z1 + z4
    out = [t10 + a3, t11 + a2, t12 + a1, t13 + a0, t13 - a0, t12 - a1, t11 - a2, t10 - a3]
    return [(o + (1 << (shift - 1))) >> shift for o in out]


def idct(d):
    """Dequantised blocks int[..., 64] (natural order) -> (samples u8[..., 8, 8], in_bound bool[...]) in 64-bit arithmetic.
    in_bound: every dequantised coefficient and every pass-1 result within +-IDCT_BOUND (the 32-bit evaluation is exact)."""
    d = np.asarray(d, np.int64).reshape(d.shape[:-1] + (8, 8))
    w = np.stack(_pass([d[..., r, :] for r in range(8)], 11), axis=-2)        # down the columns
    o = np.stack(_pass([w[..., :, c] for c in range(8)], 18), axis=-1)        # along the rows
    x = (o + 128) & 1023
    px = np.where(x < 256, x, np.where(x < 512, 255, 0)).astype(np.uint8)
    ok = (np.abs(d).max(axis=(-1, -2)) <= IDCT_BOUND) & (np.abs(w).max(axis=(-1, -2)) <= IDCT_BOUND)
    return px, ok


def planes(data, p=None):
    """Component planes at block-padded size, u8[bh*8, bw*8] each."""
    p = p or parse(data)
    out = []
    for c, q in enumerate(coefficients(data, p)):
        px, _ = idct(q.astype(np.int64) * p["quant"][c].astype(np.int64))
        bh, bw = q.shape[:2]
        out.append(px.transpose(0, 2, 1, 3).reshape(bh * 8, bw * 8))
    return out


def upsample(s, hs, vs, H, W):
    """One chroma plane (block-padded) -> int[H, W] by libjpeg's fancy upsampling."""
    dw, dh = -(-W // hs), -(-H // vs)
    s = s[:dh, :dw].astype(np.int64)
    if hs == 1:
        return s[:H, :W]
    if vs == 1:
        c, lo, hi, sh = s, 1, 2, 2
        edge0, edge1 = s[:, 0], s[:, -1]
    else:
        up, down = np.vstack([s[:1], s[:-1]]), np.vstack([s[1:], s[-1:]])
        c = np.empty((2 * dh, dw), np.int64)
        c[0::2], c[1::2] = 3 * s + up, 3 * s + down
        lo, hi, sh = 8, 7, 4
        edge0, edge1 = (4 * c[:, 0] + 8) >> 4, (4 * c[:, -1] + 7) >> 4
    out = np.empty((c.shape[0], 2 * dw), np.int64)
    left, right = np.hstack([c[:, :1], c[:, :-1]]), np.hstack([c[:, 1:], c[:, -1:]])
    out[:, 0::2] = (3 * c + left + lo) >> sh
    out[:, 1::2] = (3 * c + right + hi) >> sh
    out[:, 0], out[:, -1] = edge0, edge1
    return out[:H, :W]


def decode_strict(data, p=None, bgr=False):
    """decode, and BadStream also for a block outside the 32-bit IDCT bound (the device sets a status bit there)."""
    p = p or parse(data)
    for c, q in enumerate(coefficients(data, p)):
        if not idct(q.astype(np.int64) * p["quant"][c].astype(np.int64))[1].all():
            raise BadStream("a block outside the 32-bit IDCT bound")
    return decode(data, bgr, p)


def decode(data, bgr=False, p=None):
    """bytes -> u8[H, W, 3]."""
    p = p or parse(data)
    H, W = p["height"], p["width"]
    pl = planes(data, p)
    y = pl[0][:H, :W].astype(np.int64)
    if p["ncomp"] == 1:
        rgb = np.stack([y, y, y], -1)
    else:
        cb = upsample(pl[1], p["hs"], p["vs"], H, W) - 128
        cr = upsample(pl[2], p["hs"], p["vs"], H, W) - 128
        rgb = np.stack([y + ((91881 * cr + 32768) >> 16), y + ((-22554 * cb + 32768 - 46802 * cr) >> 16),
                        y + ((116130 * cb + 32768) >> 16)], -1)
    rgb = np.clip(rgb, 0, 255).astype(np.uint8)
    return rgb[..., ::-1].copy() if bgr else rgb
