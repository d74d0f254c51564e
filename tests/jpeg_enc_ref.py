"""The JPEG encoder's contract (include/poserisk_hip.h, section j2) restated in numpy: integer-exact, so that this file, the
kernels of csrc/jpeg_enc.hip and libjpeg's default compress path (jpeg_fdct_islow, no smoothing, the standard Huffman tables,
optimize=False: what Pillow's Image.save writes) agree on every byte.  Everything is int64 here; the kernel evaluates the
FDCT in 32 bits inside the bound `FDCT_BOUND` (tests/test_jpeg_encode_native.py compares the two at the extremes)."""
import numpy as np

from jpeg_ref import ZIGZAG

FDCT_BOUND = 35467            # PR_JPEG_FDCT_BOUND
FDCT_ROW_SUM = 60548          # the largest sum of |coefficients| over the rows of one 1-D pass as a matrix
BLOCK_BITS_MAX = 1660         # PR_JPEG_ENC_BLOCK_BITS: 11 + 11 for the DC term, 63 * (16 + 10) for the AC terms
ST_OVERFLOW = 1               # PR_JPEG_ENC_ST_OVERFLOW
SAMPLING = {"4:4:4": (1, 1), "4:2:2": (2, 1), "4:2:0": (2, 2)}

# Annex K, natural order
LUMA_Q = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51,
                   87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101,
                   72, 92, 95, 98, 112, 100, 103, 99], np.int64)
CHROMA_Q = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99,
                     99, 99, 99] + [99] * 32, np.int64)
DC_BITS = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], [0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0])
DC_VALS = (list(range(12)), list(range(12)))
AC_BITS = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d], [0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77])
AC_VALS = ([0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32,
            0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16,
            0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45,
            0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69,
            0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94,
            0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6,
            0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8,
            0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8,
            0xf9, 0xfa],
           [0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81,
            0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34,
            0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44,
            0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68,
            0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92,
            0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4,
            0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6,
            0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8,
            0xf9, 0xfa])


def quant_tables(quality):
    """-> int64[2, 64], natural order: Annex K scaled by libjpeg's jpeg_quality_scaling, clamped to 1..255 (baseline)."""
    q = int(quality)
    assert 1 <= q <= 100
    scale = 5000 // q if q < 50 else 200 - 2 * q
    return np.stack([np.clip((base * scale + 50) // 100, 1, 255) for base in (LUMA_Q, CHROMA_Q)])


def huff_codes(bits, vals):
    """-> {symbol: (code, length)} by the standard's Annex C."""
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return out


def geometry(H, W, hs, vs, restart_interval):
    """-> (mx, my, MCUs per restart segment or 0): restart_interval -1 = one MCU row; libjpeg keeps at most 65535."""
    mx, my = -(-W // (8 * hs)), -(-H // (8 * vs))
    ri = mx if restart_interval < 0 else int(restart_interval)
    return mx, my, min(ri, 65535)


def header(H, W, quality, hs, vs, restart_interval):
    """Everything up to and including SOS, as libjpeg writes it."""
    _, _, ri = geometry(H, W, hs, vs, restart_interval)
    qt = quant_tables(quality)
    out = bytearray(b"\xff\xd8\xff\xe0\x00\x10JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    for t in range(2):
        out += b"\xff\xdb\x00\x43" + bytes([t]) + bytes(int(v) for v in qt[t][ZIGZAG])
    out += b"\xff\xc0\x00\x11\x08" + bytes([H >> 8, H & 255, W >> 8, W & 255, 3, 1, hs << 4 | vs, 0, 2, 0x11, 1, 3, 0x11, 1])
    for t in range(2):
        for cls, (bits, vals) in enumerate(((DC_BITS[t], DC_VALS[t]), (AC_BITS[t], AC_VALS[t]))):
            n = 2 + 1 + 16 + len(vals)
            out += b"\xff\xc4" + bytes([n >> 8, n & 255, cls << 4 | t]) + bytes(bits) + bytes(vals)
    if ri:
        out += b"\xff\xdd\x00\x04" + bytes([ri >> 8, ri & 255])
    out += b"\xff\xda\x00\x0c\x03\x01\x00\x02\x11\x03\x11\x00\x3f\x00"
    return bytes(out)


def ycc(img, bgr=False):
    rgb = np.asarray(img)[..., ::-1] if bgr else np.asarray(img)
    R, G, B = (rgb[..., i].astype(np.int64) for i in range(3))
    return ((19595 * R + 38470 * G + 7471 * B + 32768) >> 16,
            (-11059 * R - 21709 * G + 32768 * B + (128 << 16) + 32767) >> 16,
            (32768 * R - 27439 * G - 5329 * B + (128 << 16) + 32767) >> 16)


def component_planes(img, hs, vs, bgr=False):
    """-> [Y, Cb, Cr] at MCU-padded size, in the contract's order: right column out to the padded width, bottom row up to a
    multiple of vs, downsample, then the last downsampled row down to the MCU rows' height."""
    H, W = img.shape[:2]
    mx, my, _ = geometry(H, W, hs, vs, 0)
    Y, Cb, Cr = ycc(img, bgr)
    out = [np.pad(Y, ((0, my * 8 * vs - H), (0, mx * 8 * hs - W)), mode="edge")]
    for c in (Cb, Cr):
        c = np.pad(c, ((0, -H % vs), (0, mx * 8 * hs - W)), mode="edge")
        if (hs, vs) == (2, 2):
            d = (c[0::2, 0::2] + c[0::2, 1::2] + c[1::2, 0::2] + c[1::2, 1::2] + np.tile([1, 2], mx * 4)) >> 2
        elif (hs, vs) == (2, 1):
            d = (c[:, 0::2] + c[:, 1::2] + np.tile([0, 1], mx * 4)) >> 1
        else:
            d = c
        out.append(np.pad(d, ((0, my * 8 - d.shape[0]), (0, 0)), mode="edge"))
    return out


def _pass(d, first):
    """One 1-D pass of jfdctint.c along the last axis."""
    d0, d1, d2, d3, d4, d5, d6, d7 = (d[..., i] for i in range(8))
    t0, t7, t1, t6, t2, t5, t3, t4 = d0 + d7, d0 - d7, d1 + d6, d1 - d6, d2 + d5, d2 - d5, d3 + d4, d3 - d4
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    n = 11 if first else 15

    def descale(x, s):
        return (x + (1 << (s - 1))) >> s
    o = [None] * 8
    o[0] = (t10 + t11) << 2 if first else descale(t10 + t11, 2)
    o[4] = (t10 - t11) << 2 if first else descale(t10 - t11, 2)
    z1 = (t12 + t13) * 4433
    o[2] = descale(z1 + t13 * 6270, n)
    o[6] = descale(z1 - t12 * 15137, n)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * 9633
    t4, t5, t6, t7 = t4 * 2446, t5 * 16819, t6 * 25172, t7 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    o[7], o[5], o[3], o[1] = descale(t4 + z1 + z3, n), descale(t5 + z2 + z4, n), descale(t6 + z2 + z3, n), descale(t7 + z1 + z4, n)
    return np.stack(o, -1)


def fdct(samples, with_pass1=False):
    """samples int[..., 8, 8] (0..255) -> coefficients int64[..., 8, 8] (scaled by 8, as jpeg_fdct_islow leaves them)."""
    p1 = _pass(np.asarray(samples, np.int64) - 128, True)                       # rows
    out = np.swapaxes(_pass(np.swapaxes(p1, -1, -2), False), -1, -2)            # columns
    return (out, p1) if with_pass1 else out


def quantise(c, q):
    """c int64[..., 64] (natural order), q int64[64] -> (|c| + q8 / 2) / q8 with the sign restored, q8 = 8 q."""
    q8 = 8 * np.asarray(q, np.int64)
    m = (np.abs(c) + (q8 >> 1)) // q8
    return np.where(c < 0, -m, m)


def mcu_blocks(img, quality, hs, vs, bgr=False):
    """-> int64[n MCUs, hs * vs + 2, 64]: quantised coefficients in ZIG-ZAG order, MCU by MCU, dummy blocks resolved."""
    H, W = img.shape[:2]
    mx, my, _ = geometry(H, W, hs, vs, 0)
    qt = quant_tables(quality)
    comps = []
    for ci, p in enumerate(component_planes(img, hs, vs, bgr)):
        bh, bw = p.shape[0] // 8, p.shape[1] // 8
        blocks = p.reshape(bh, 8, bw, 8).transpose(0, 2, 1, 3)
        comps.append(quantise(fdct(blocks).reshape(bh, bw, 64), qt[min(ci, 1)])[..., ZIGZAG])
    luma = comps[0].reshape(my, vs, mx, hs, 64).transpose(0, 2, 1, 3, 4).reshape(my * mx, vs * hs, 64)
    by, bx = np.mgrid[0:my * vs, 0:mx * hs]
    dummy = ((by >= -(-H // 8)) | (bx >= -(-W // 8))).reshape(my, vs, mx, hs).transpose(0, 2, 1, 3).reshape(my * mx, vs * hs)
    for k in range(1, hs * vs):                              # in MCU order, so that a run of dummies copies one DC along
        luma[:, k, 1:][dummy[:, k]] = 0
        luma[:, k, 0] = np.where(dummy[:, k], luma[:, k - 1, 0], luma[:, k, 0])
    assert not dummy[:, 0].any()
    return np.concatenate([luma, comps[1].reshape(-1, 1, 64), comps[2].reshape(-1, 1, 64)], 1)


class _Writer:
    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    def put(self, code, length):
        self.acc = (self.acc << length) | code
        self.n += length
        while self.n >= 8:
            self.n -= 8
            self.out.append((self.acc >> self.n) & 255)
        self.acc &= (1 << self.n) - 1

    def flush(self):
        if self.n:
            self.put((1 << (8 - self.n)) - 1, 8 - self.n)
        data, self.out = bytes(self.out).replace(b"\xff", b"\xff\x00"), bytearray()
        return data


def block_bits(block, pred, dc, ac, w=None):
    """One block as jchuff.c's encode_one_block codes it -> its bit count; the bits go to `w` when given."""
    bits = 0

    def put(code, length):
        nonlocal bits
        bits += length
        if w is not None:
            w.put(code, length)
    diff = int(block[0]) - pred
    n = abs(diff).bit_length()
    put(*dc[n])
    if n:
        put((diff if diff >= 0 else diff - 1) & ((1 << n) - 1), n)
    run = 0
    nz = np.nonzero(block[1:])[0] + 1
    last = 0
    for k in nz:
        run = int(k) - last - 1
        while run > 15:
            put(*ac[0xF0])
            run -= 16
        v = int(block[k])
        n = abs(v).bit_length()
        put(*ac[run << 4 | n])
        put((v if v >= 0 else v - 1) & ((1 << n) - 1), n)
        last = int(k)
    if last != 63:
        put(*ac[0])
    return bits


def encode(img, quality=90, subsampling="4:2:0", restart_interval=0, bgr=False):
    """img u8[H, W, 3] -> the complete baseline JPEG file (bytes)."""
    hs, vs = SAMPLING[subsampling]
    H, W = img.shape[:2]
    _, _, ri = geometry(H, W, hs, vs, restart_interval)
    mcus = mcu_blocks(img, quality, hs, vs, bgr)
    dc = [huff_codes(DC_BITS[t], DC_VALS[t]) for t in range(2)]
    ac = [huff_codes(AC_BITS[t], AC_VALS[t]) for t in range(2)]
    out, w, pred, rst = bytearray(header(H, W, quality, hs, vs, restart_interval)), _Writer(), [0, 0, 0], 0
    nl = hs * vs
    for m, blocks in enumerate(mcus):
        if ri and m and m % ri == 0:
            out += w.flush() + bytes([0xFF, 0xD0 + rst])
            rst, pred = (rst + 1) & 7, [0, 0, 0]
        for k, b in enumerate(blocks):
            c = max(k - nl + 1, 0)
            block_bits(b, pred[c], dc[min(c, 1)], ac[min(c, 1)], w)
            pred[c] = int(b[0])
    return bytes(out + w.flush() + b"\xff\xd9")


def encode_bound(H, W, hs, vs, restart_interval):
    """pr_jpeg_encode_bound: header + every block at BLOCK_BITS_MAX with every byte stuffed + a pad byte and a marker per segment."""
    mx, my, ri = geometry(H, W, hs, vs, restart_interval)
    nmcu = mx * my
    nseg = -(-nmcu // ri) if ri else 1
    return len(header(H, W, 1, hs, vs, restart_interval)) + nmcu * (hs * vs + 2) * BLOCK_BITS_MAX // 4 + 4 * nseg + 2
