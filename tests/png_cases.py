"""Inputs of the PNG decoder's tests, all made here: a minimal PNG writer on zlib.compressobj (so that the module controls the
deflate stream: level, strategy, flushes, how the stream is cut into IDAT chunks), a stored-only writer, a hand-made dynamic
block writer for the code sets zlib never emits, and the bad-stream list.  No fixture files, nothing from outside.

The module asserts its own coverage when it is imported, by walking every small stream with the reference inflate
(tests/png_ref.py): block types 0, 1 and 2, a length-258 match, a distance of 32 000 or more, overlapping matches
(distance < length) at distances 1, 2, 3, 63, 64 and 65, a code longer than the first-level table, a dynamic block with a
single distance code, and dynamic blocks without a match (with and without a distance code)."""
import functools
import struct
import zlib

import numpy as np

import png_ref as ref

SIZES = ((1, 1), (1, 7), (7, 1), (5, 3), (33, 17), (160, 90))   # (W, H)
COLOR_TYPES = (0, 2, 3, 4, 6)
ADAPTIVE = 5


def chunk(typ, body):
    return struct.pack(">I", len(body)) + typ + body + struct.pack(">I", zlib.crc32(typ + body))


def _paeth_vec(a, b, c):
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    return np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))


def filter_rows(px, bpp, mode):
    """u8[H, W * bpp] -> the filtered scanlines (bytes), filter `mode` on every row, or ADAPTIVE: row y gets filter y % 5 for the
    first ten rows and the minimum-sum-of-absolute-differences choice after that."""
    px = px.astype(np.int64)
    H, n = px.shape
    left = np.zeros_like(px)
    left[:, bpp:] = px[:, :-bpp] if n > bpp else 0
    up = np.zeros_like(px)
    up[1:] = px[:-1]
    ul = np.zeros_like(px)
    ul[1:, bpp:] = px[:-1, :-bpp] if n > bpp else 0
    forms = [px, px - left, px - up, px - ((left + up) >> 1), px - _paeth_vec(left, up, ul)]
    forms = [(f & 255).astype(np.uint8) for f in forms]
    out = bytearray()
    for y in range(H):
        if mode == ADAPTIVE:
            ft = y % 5 if y < 10 else int(np.argmin([np.abs(f[y].astype(np.int8).astype(np.int64)).sum() for f in forms]))
        else:
            ft = mode
        out += bytes([ft]) + forms[ft][y].tobytes()
    return bytes(out)


def deflate(raw, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, flush_at=()):
    c = zlib.compressobj(level, zlib.DEFLATED, 15, 9, strategy)
    out, at = b"", 0
    for cut in flush_at:
        out += c.compress(raw[at:cut]) + c.flush(zlib.Z_FULL_FLUSH)
        at = cut
    return out + c.compress(raw[at:]) + c.flush()


def stored(raw, block=65535):
    """A zlib stream of stored blocks only (what a writer without a compressor emits)."""
    out = b"\x78\x01"
    blocks = [raw[i:i + block] for i in range(0, len(raw), block)] or [b""]
    for i, part in enumerate(blocks):
        out += bytes([i == len(blocks) - 1]) + struct.pack("<HH", len(part), len(part) ^ 0xFFFF) + part
    return out + struct.pack(">I", zlib.adler32(raw))


class _BitWriter:
    def __init__(self):
        self.v, self.n = 0, 0

    def put(self, value, bits):
        self.v |= value << self.n
        self.n += bits

    def code(self, code, length):   # Huffman codes go most significant bit first
        self.put(int(format(code, f"0{length}b")[::-1], 2) if length else 0, length)

    def bytes(self):
        return self.v.to_bytes((self.n + 7) // 8, "little")


def _canonical(lens):
    codes, code = {}, 0
    for ln in range(1, 16):
        for s, x in enumerate(lens):
            if x == ln:
                codes[s] = (code, ln)
                code += 1
        code <<= 1
    return codes


def dynamic_block_stream(raw, lit_lens, dist_lens, tokens):
    """A zlib stream of ONE dynamic block with the given code lengths (286 literal/length, up to 30 distance) and tokens: ints
    (literals) and (length symbol, extra value, distance symbol, extra value) tuples.  The code-length code is sixteen codes
    of four bits for the lengths 0..15, no repeat codes."""
    w = _BitWriter()
    w.put(1, 1)
    w.put(2, 2)
    w.put(len(lit_lens) - 257, 5)
    w.put(len(dist_lens) - 1, 5)
    w.put(19 - 4, 4)
    for s in ref.CL_ORDER:
        w.put(4 if s < 16 else 0, 3)
    for x in list(lit_lens) + list(dist_lens):
        w.code(x, 4)                          # sixteen 4-bit codes: the code of length value x is x
    lit, dst = _canonical(lit_lens), _canonical(dist_lens)
    for t in tokens:
        if isinstance(t, int):
            w.code(*lit[t])
        else:
            ls, lx, ds, dx = t
            w.code(*lit[ls])
            w.put(lx, ref.LEN_EXTRA[ls - 257])
            w.code(*dst[ds])
            w.put(dx, ref.DIST_EXTRA[ds])
    w.code(*lit[256])
    return b"\x78\x9c" + w.bytes() + struct.pack(">I", zlib.adler32(raw))


def png(W, H, color_type, z, palette=None, idat=None, extra=()):
    """The file around a zlib stream.  idat: None (one chunk), an int n (chunks of n bytes), or "empties" (chunks of 5 bytes with
    an empty chunk in front of, between and behind them).  extra: ancillary chunks (type, body) placed behind IHDR."""
    out = ref.SIGNATURE + chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, color_type, 0, 0, 0))
    for typ, body in extra:
        out += chunk(typ, body)
    if palette is not None:
        out += chunk(b"PLTE", bytes(palette))
    if idat is None:
        parts = [z]
    elif idat == "empties":
        parts = [b""]
        for i in range(0, len(z), 5):
            parts += [z[i:i + 5], b""]
    else:
        parts = [z[i:i + idat] for i in range(0, len(z), idat)]
    return out + b"".join(chunk(b"IDAT", p) for p in parts) + chunk(b"IEND", b"")


def _rng(*key):
    return np.random.default_rng([int(k) & 0xFFFFFFFF for k in key])


def pixels_for(W, H, color_type, seed, kind="smooth"):
    """Source samples u8[H, W * bpp] and, for colour type 3, a palette (bytes, 3 * entries)."""
    r = _rng(W, H, color_type, seed)
    bpp = ref.BPP[color_type]
    if kind == "noise":
        px = r.integers(0, 256, (H, W * bpp), dtype=np.uint8)
    else:
        y, x = np.mgrid[0:H, 0:W * bpp]
        px = ((x * 3 + y * 5 + seed * 7) % 256 + r.integers(0, 6, (H, W * bpp))).astype(np.uint8)
    palette = None
    if color_type == 3:
        n = 256 if seed % 2 else 77                      # a short palette: indices past it read black
        palette = r.integers(0, 256, 3 * n, dtype=np.uint8).tobytes()
    return px, palette


def expected_rgb(px, W, H, color_type, palette):
    fr = dict(width=W, height=H, color_type=color_type, bpp=ref.BPP[color_type],
              palette=None if palette is None else bytes(palette) + bytes(768 - len(palette)))
    return ref.colour(px, fr)


def _case(name, W, H, ct, px, palette, mode, z_of, idat=None, extra=()):
    raw = filter_rows(px, ref.BPP[ct], mode)
    return name, png(W, H, ct, z_of(raw), palette, idat, extra), expected_rgb(px, W, H, ct, palette)


def _special_160x90():
    """The 160 x 90 cases whose streams are built for one property each -> [(name, file, expected rgb)]."""
    W, H, out = 160, 90, []
    r = _rng(160, 90, 99)
    # a copy 67 rows up in noise: distance 67 * 481 = 32 227
    px = r.integers(0, 256, (H, W * 3), dtype=np.uint8)
    px[67:69] = px[0:2]
    out.append(_case("160x90 rgb far-copy level9", W, H, 2, px, None, 0, lambda raw: deflate(raw, 9)))
    # rows of fresh random periods: overlapping matches at distance = period
    px = np.zeros((H, W), np.uint8)
    for y in range(H):
        period = (1, 2, 3, 63, 64, 65)[y % 6]
        px[y] = np.resize(r.integers(0, 256, period, dtype=np.uint8), W)
    out.append(_case("160x90 gray periods level9", W, H, 0, px, None, 0, lambda raw: deflate(raw, 9)))
    # runs far longer than 64 under Z_RLE: distance-1 copies of 258
    px = np.repeat(r.integers(0, 256, (H, 2), dtype=np.uint8), W // 2, axis=1)
    out.append(_case("160x90 gray runs rle", W, H, 0, px, None, 0, lambda raw: deflate(raw, 6, zlib.Z_RLE)))
    # a geometric byte distribution under Z_HUFFMAN_ONLY: codes of up to 15 bits, and a dynamic block without a match
    px = np.minimum(r.geometric(0.5, (H, W * 4)) - 1, 40).astype(np.uint8) * 6
    out.append(_case("160x90 rgba skewed huffman-only", W, H, 6, px, None, 0, lambda raw: deflate(raw, 6, zlib.Z_HUFFMAN_ONLY)))
    px, pal = pixels_for(W, H, 3, 1)
    out.append(_case("160x90 palette level1 idat7", W, H, 3, px, pal, ADAPTIVE, lambda raw: deflate(raw, 1), idat=7))
    px, _ = pixels_for(W, H, 4, 2)
    out.append(_case("160x90 gray-alpha fixed", W, H, 4, px, None, 4, lambda raw: deflate(raw, 6, zlib.Z_FIXED)))
    px, _ = pixels_for(W, H, 6, 3, "noise")
    out.append(_case("160x90 rgba stored", W, H, 6, px, None, 3, stored))
    px, _ = pixels_for(W, H, 2, 4)
    out.append(_case("160x90 rgb adaptive level6 full-flush", W, H, 2, px, None, ADAPTIVE,
                     lambda raw: deflate(raw, 6, flush_at=(1000, 1000, 20011))))
    px, _ = pixels_for(W, H, 2, 5)
    out.append(_case("160x90 rgb paeth level0", W, H, 2, px, None, 4, lambda raw: deflate(raw, 0)))
    # hand-made dynamic blocks.  One distance code of one bit (an incomplete set zlib accepts): every row repeats the row's
    # first byte, as a literal and matches of 258 / rest at distance 1.
    px = np.repeat(r.integers(0, 256, (H, 1), dtype=np.uint8), W, axis=1)
    raw = filter_rows(px, 1, 0)
    lit = [9] * 256 + [2] + [0] * 29                  # literals 9 bits, end of block 2, length symbols 277 and 285 3 bits: complete
    lit[277] = lit[285] = 3
    tokens, i = [], 0
    while i < len(raw):
        run = 1
        while i + run < len(raw) and raw[i + run] == raw[i]:
            run += 1
        tokens.append(raw[i])
        left = run - 1
        while left >= 67:                              # 258 by symbol 285, 67..82 by symbol 277 and four extra bits
            n = 258 if left >= 258 else min(left, 82)
            tokens.append((285, 0, 0, 0) if n == 258 else (277, n - 67, 0, 0))
            left -= n
        tokens += [raw[i]] * left
        i += run
    z = dynamic_block_stream(raw, lit, [1], tokens)
    out.append(("160x90 gray single-distance-code", png(W, H, 0, z), expected_rgb(px, W, H, 0, None)))
    # no distance code at all (HDIST = 1, length 0): literals of 9 bits and a 1-bit end of block
    px, _ = pixels_for(W, H, 0, 6, "noise")
    raw = filter_rows(px, 1, 0)
    z = dynamic_block_stream(raw, [9] * 256 + [1], [0], list(raw))
    out.append(("160x90 gray no-distance-code", png(W, H, 0, z), expected_rgb(px, W, H, 0, None)))
    return out


@functools.lru_cache(maxsize=None)
def small_cases():
    """[(name, file bytes, expected u8[H, W, 3] RGB)]; names start with "<W>x<H> "."""
    out = []
    for W, H in SIZES[:5]:
        for ct in COLOR_TYPES:
            for mode in range(6):
                px, pal = pixels_for(W, H, ct, mode)
                out.append(_case(f"{W}x{H} ct{ct} filter{mode} level6", W, H, ct, px, pal, mode, deflate))
    W, H = 33, 17
    px, _ = pixels_for(W, H, 2, 11)
    kinds = (("level0", lambda raw: deflate(raw, 0), None), ("fixed", lambda raw: deflate(raw, 6, zlib.Z_FIXED), None),
             ("level1", lambda raw: deflate(raw, 1), None), ("level9", lambda raw: deflate(raw, 9), None),
             ("huffman-only", lambda raw: deflate(raw, 6, zlib.Z_HUFFMAN_ONLY), None),
             ("rle", lambda raw: deflate(raw, 6, zlib.Z_RLE), None),
             ("full-flush", lambda raw: deflate(raw, 6, flush_at=(100, 100, 700)), None),
             ("stored", stored, None), ("level6 idat1", deflate, 1), ("level6 idat7", deflate, 7), ("level6 empties", deflate, "empties"))
    for name, z_of, idat in kinds:
        out.append(_case(f"33x17 ct2 adaptive {name}", W, H, 2, px, None, ADAPTIVE, z_of, idat))
    out.append(_case("33x17 ct2 adaptive level6 ancillary", W, H, 2, px, None, ADAPTIVE, deflate,
                     extra=((b"gAMA", struct.pack(">I", 45455)), (b"tRNS", bytes(6)), (b"tEXt", b"Comment\0made here"))))
    # the first IDAT payload at a 16-aligned offset of the file (8 + 25 + 23 + 8 = 64): alone in a call, the gather's 16-byte
    # path starts on its first byte; in the other cases it starts behind a head of 1..15 bytes
    pad = ((b"tEXt", b"Comment\0pad"),)
    out.append(_case("33x17 ct2 adaptive level6 idat-at-64", W, H, 2, px, None, ADAPTIVE, deflate, extra=pad))
    big, _ = pixels_for(160, 90, 2, 12, "noise")
    aligned = [_case("160x90 rgb noise level6 idat-at-64", 160, 90, 2, big, None, 0, deflate, extra=pad),
               _case("160x90 rgb noise level6 idat-at-64 in 4 KiB chunks", 160, 90, 2, big, None, 2, deflate, idat=4096, extra=pad)]
    for name, blob, _ in [out[-1]] + aligned:
        assert ref.parse(blob)["idat"][0][0] == 64, name
    return tuple(out + _special_160x90() + aligned)


def by_size():
    """{(W, H): [case]} in SIZES' order."""
    groups = {s: [] for s in SIZES}
    for c in small_cases():
        w, h = c[0].split(" ")[0].split("x")
        groups[(int(w), int(h))].append(c)
    return groups


@functools.lru_cache(maxsize=None)
def large_frames():
    """Three 800 x 450 RGB frames -> [(name, file, expected rgb)]: a synthetic scene at Pillow-like settings (adaptive filters,
    level 6, 64 KiB IDATs), the same at level 1 in 8 KiB IDATs, and noise by the stored-only writer (more than 65 535 bytes: many
    stored blocks)."""
    W, H = 800, 450
    y, x = np.mgrid[0:H, 0:W]
    scene = np.stack([(x * 255 // W), (y * 255 // H), ((x // 16 + y // 16) % 2) * 200], axis=2).astype(np.int64)
    scene = (scene + _rng(800, 450, 1).integers(0, 12, scene.shape)).clip(0, 255).astype(np.uint8).reshape(H, W * 3)
    noise = _rng(800, 450, 2).integers(0, 256, (H, W * 3), dtype=np.uint8)
    return (_case("800x450 scene level6", W, H, 2, scene, None, ADAPTIVE, deflate, idat=65536),
            _case("800x450 scene level1", W, H, 2, scene[::-1].copy(), None, 4, lambda raw: deflate(raw, 1), idat=8192),
            _case("800x450 noise stored", W, H, 2, noise, None, 0, stored))


# ---- the bad-stream list -------------------------------------------------------------------------------------------------
FUZZ_W, FUZZ_H = 33, 17


@functools.lru_cache(maxsize=None)
def fuzz_base():
    """(zlib stream, raw size) of one small dynamic stream: 33 x 17 RGB, adaptive filters, level 9."""
    px, _ = pixels_for(FUZZ_W, FUZZ_H, 2, 21)
    raw = filter_rows(px, 3, ADAPTIVE)
    z = deflate(raw, 9)
    assert ref.inflate(z, len(raw))[3]["blocks"] == [2]
    return z, len(raw)


def wrap(z, W=FUZZ_W, H=FUZZ_H, color_type=2):
    """A damaged zlib stream in a well-formed file (right CRCs), so that the damage reaches the inflate."""
    return png(W, H, color_type, z)


def xor_mutations(z):
    """Every single-byte XOR of z with one bit pattern per byte (seeded), as zlib streams."""
    r = _rng(len(z), 7)
    masks = r.integers(1, 256, len(z))
    return [z[:i] + bytes([z[i] ^ int(masks[i])]) + z[i + 1:] for i in range(len(z))]


def truncations(z):
    return [z[:i] for i in range(len(z))]


def corruptions(z, n=2000):
    """n seeded corruptions: one to three bytes replaced, or a byte dropped or doubled, behind the zlib header."""
    r = _rng(len(z), n, 13)
    out = []
    for _ in range(n):
        b, kind = bytearray(z), int(r.integers(0, 4))
        if kind < 2:
            for _ in range(int(r.integers(1, 4))):
                b[int(r.integers(2, len(b)))] = int(r.integers(0, 256))
        elif kind == 2:
            del b[int(r.integers(2, len(b)))]
        else:
            i = int(r.integers(2, len(b)))
            b.insert(i, b[i])
        out.append(bytes(b))
    return out


@functools.lru_cache(maxsize=None)
def gpu_bad_files():
    """Six bad files of 160 x 90 RGB, one for each status bit -> [(name, file, the status bit)].  tests/test_png_cpu.py proves the
    reference's verdict on each against zlib and tests/test_png_native.py runs the same bytes under sanitizers before
    tests/test_png_gpu.py decodes them once."""
    W, H = 160, 90
    px, _ = pixels_for(W, H, 2, 31)
    raw = filter_rows(px, 3, ADAPTIVE)
    z = deflate(raw, 6)
    good = png(W, H, 2, z)
    crc_hit = bytearray(good)
    crc_hit[len(good) // 2] ^= 0x40                                           # inside IDAT: the chunk's CRC no longer matches
    # a distance before the start of the output: a fixed block whose first token is a match (length 3, distance 1)
    w = _BitWriter()
    w.put(1, 1)
    w.put(1, 2)
    w.code(0b0000001, 7)                                                       # length symbol 257
    w.code(0, 5)                                                               # distance symbol 0
    too_far = b"\x78\x9c" + w.bytes() + bytes(4)
    longer = filter_rows(np.concatenate([px, px[:1]]), 3, 0)                   # one row too many: the output would overrun
    bad_filter = bytearray(raw)
    bad_filter[5 * (1 + W * 3)] = 7
    wrong_sum = bytearray(z)
    wrong_sum[-1] ^= 1
    return (("refused: CRC", bytes(crc_hit), ref.ST_REFUSED), ("truncated", png(W, H, 2, z[:len(z) * 2 // 3]), ref.ST_TRUNCATED),
            ("bad code: distance before the start", png(W, H, 2, too_far), ref.ST_BAD_CODE),
            ("size: output overruns", png(W, H, 2, deflate(longer, 6)), ref.ST_SIZE),
            ("filter byte 7", png(W, H, 2, deflate(bytes(bad_filter), 6)), ref.ST_FILTER),
            ("checksum", png(W, H, 2, bytes(wrong_sum)), ref.ST_CHECKSUM))


def _assert_coverage():
    blocks, lengths, overlaps, far, long_codes, single, no_match, no_dist = set(), set(), set(), 0, 0, 0, 0, 0
    for name, blob, _ in small_cases():
        fr = ref.parse(blob)
        assert fr["status"] == 0, name
        z = b"".join(blob[b:e] for b, e in fr["idat"])
        st, _, _, info = ref.inflate(z, fr["height"] * (1 + fr["width"] * fr["bpp"]))
        assert st == 0, (name, st)
        blocks |= set(info["blocks"])
        long_codes += info["long_codes"]
        for ln, d in info["matches"]:
            lengths.add(ln)
            far = max(far, d)
            if d < ln:
                overlaps.add(d)
        for ndist, nmatch in info["dyn"]:
            single += ndist == 1 and nmatch > 0
            no_match += nmatch == 0
            no_dist += ndist == 0
    assert blocks == {0, 1, 2}, blocks
    assert 258 in lengths and far >= 32000, (max(lengths), far)
    assert {1, 2, 3, 63, 64, 65} <= overlaps, sorted(overlaps)
    assert long_codes > 0 and single > 0 and no_match > 0 and no_dist > 0, (long_codes, single, no_match, no_dist)


_assert_coverage()
