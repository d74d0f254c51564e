"""The PNG encoder's contract (include/poserisk_hip.h, section j5) restated in numpy and Python: the filters, the adaptive
choice, the 16 KiB segments, zlib's deflate_rle token rule, the code construction with its length limiter, the code-length
code, the stored fallback and the file layout.  The checksums come from zlib here (crc32, adler32), so that the kernels'
parallel combination is compared with an independent serial one.  Nothing here is shared with the library."""
import struct
import zlib

import numpy as np

SEGMENT = 16384
MAX_SIDE = 4096
STORED, RLE = 0, 1
ADAPTIVE = 5
ST_OVERFLOW = 1
ZLIB_HEADER = b"\x78\x01"
SIGNATURE = b"\x89PNG\r\n\x1a\n"
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
LEN_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
LEN_EXTRA = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)


def bound(H, W):
    """No file of an H x W frame is larger: 63 fixed bytes, and every segment at most its bytes and a 5-byte stored header."""
    raw = H * (1 + 3 * W)
    return 63 + raw + 5 * (-(-raw // SEGMENT))


# ---- filters ---------------------------------------------------------------------------------------------------------------
def _paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    return np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))


def filter_rows(px, filt):
    """u8[H,W,3] RGB -> (the filtered stream u8[H (1 + 3 W)], the filter of every row).  a, b, c come from the RAW rows."""
    H, W, _ = px.shape
    raw = px.reshape(H, 3 * W).astype(np.int32)
    out = np.zeros((H, 1 + 3 * W), np.uint8)
    types = np.zeros(H, np.int32)
    zero = np.zeros(3 * W, np.int32)
    for r in range(H):
        x, b = raw[r], raw[r - 1] if r else zero
        a = np.concatenate([zero[:3], x[:-3]])[:3 * W]
        c = np.concatenate([zero[:3], b[:-3]])[:3 * W]
        cand = [x, x - a, x - b, x - ((a + b) >> 1), x - _paeth(a, b, c)]
        cand = [(v & 255).astype(np.int32) for v in cand]
        if filt == ADAPTIVE:
            cost = [int(np.where(v < 128, v, 256 - v).sum()) for v in cand]
            t = cost.index(min(cost))                            # ties: the lowest filter number
        else:
            t = filt
        types[r] = t
        out[r, 0] = t
        out[r, 1:] = cand[t]
    return out.reshape(-1), types


# ---- code construction -----------------------------------------------------------------------------------------------------
def code_lengths(hist, limit):
    """-> (length per symbol, whether the limiter acted).  Used symbols in (count, symbol) order; a two-queue Huffman merge
    (of two equal weights the internal node is taken before the leaf, internal nodes in the order they were made) gives the
    number of codes per depth; depths above `limit` are moved to `limit` and the Kraft sum is repaired one unit at a time:
    drop one code of length `limit`, take one code of the greatest length d < limit that has any and make it two of d + 1.
    The lengths are then handed out longest first in (count, symbol) order."""
    used = sorted((c, s) for s, c in enumerate(hist) if c)
    n = len(used)
    lens = [0] * len(hist)
    if n == 0:
        return lens, False
    if n == 1:
        lens[used[0][1]] = 1
        return lens, False
    w = [c for c, _ in used] + [0] * (n - 1)
    parent = [0] * (2 * n - 1)
    leaf, ihead = 0, n
    for k in range(n, 2 * n - 1):
        pair = []
        for _ in range(2):
            if leaf < n and (ihead >= k or w[leaf] < w[ihead]):
                pair.append(leaf)
                leaf += 1
            else:
                pair.append(ihead)
                ihead += 1
        w[k] = w[pair[0]] + w[pair[1]]
        parent[pair[0]] = parent[pair[1]] = k
    depth = [0] * (2 * n - 1)
    for i in range(2 * n - 3, -1, -1):
        depth[i] = depth[parent[i]] + 1
    count = [0] * (limit + 1)
    limited = False
    for i in range(n):
        limited |= depth[i] > limit
        count[min(depth[i], limit)] += 1
    total = sum(count[d] << (limit - d) for d in range(1, limit + 1))
    while total > (1 << limit):
        count[limit] -= 1
        for d in range(limit - 1, 0, -1):
            if count[d]:
                count[d] -= 1
                count[d + 1] += 2
                break
        total -= 1
    j = 0
    for d in range(limit, 0, -1):
        for _ in range(count[d]):
            lens[used[j][1]] = d
            j += 1
    return lens, limited


def canonical(lens):
    """RFC 1951 3.2.2 -> the code of every symbol, already bit-reversed (deflate sends Huffman codes most significant bit first)."""
    maxl = max(lens) if lens else 0
    bl = [0] * (maxl + 2)
    for v in lens:
        if v:
            bl[v] += 1
    nxt, code = [0] * (maxl + 2), 0
    for b in range(1, maxl + 1):
        code = (code + bl[b - 1]) << 1
        nxt[b] = code
    out = [0] * len(lens)
    for s, v in enumerate(lens):
        if v:
            out[s] = int(format(nxt[v], f"0{v}b")[::-1], 2)
            nxt[v] += 1
    return out


def length_sequence(seq):
    """The code-length code's symbols for a sequence of lengths: [(symbol, extra value, extra bits)].  A run of zeros: while at
    least 3 remain, 18 for min(run, 138) when at least 11 remain, else 17; fewer than 3 go out as they are.  A run of a non-zero
    length: the length itself once, then 16 for min(rest, 6) while at least 3 remain, then the rest as they are."""
    out, i = [], 0
    while i < len(seq):
        v, j = seq[i], i
        while j < len(seq) and seq[j] == v:
            j += 1
        run = j - i
        if v == 0:
            while run >= 3:
                if run >= 11:
                    k = min(run, 138)
                    out.append((18, k - 11, 7))
                else:
                    k = run
                    out.append((17, k - 3, 3))
                run -= k
        else:
            out.append((v, 0, 0))
            run -= 1
            while run >= 3:
                k = min(run, 6)
                out.append((16, k - 3, 2))
                run -= k
        out.extend([(v, 0, 0)] * run)
        i = j
    return out


# ---- one segment -----------------------------------------------------------------------------------------------------------
def tokens(seg):
    """zlib's deflate_rle rule on one segment -> (positions of literals, positions of matches, their lengths)."""
    n = len(seg)
    start = np.ones(n, bool)
    start[1:] = seg[1:] != seg[:-1]
    first = np.maximum.accumulate(np.where(start, np.arange(n), 0))
    ends = np.append(np.nonzero(start)[0][1:], n)
    length = ends[np.cumsum(start) - 1] - first
    o = np.arange(n) - first
    r, R = o - 1, length - 1
    blk = (r // 258) * 258
    blen = np.minimum(258, R - blk)
    lit = (o == 0) | (blen < 3)
    match = (o > 0) & (blen >= 3) & (r == blk)
    return np.nonzero(lit)[0], np.nonzero(match)[0], blen[match]


def _pack(vals, nbits):
    vals, nbits = np.asarray(vals, np.int64), np.asarray(nbits, np.int64)
    idx = np.repeat(np.arange(len(vals)), nbits)
    within = np.arange(int(nbits.sum())) - np.repeat(np.cumsum(nbits) - nbits, nbits)
    return np.packbits(((vals[idx] >> within) & 1).astype(np.uint8), bitorder="little").tobytes(), int(nbits.sum())


def stored_segment(seg, last):
    n = len(seg)
    return bytes([1 if last else 0]) + struct.pack("<HH", n, n ^ 0xFFFF) + bytes(seg)


def encode_segment(seg, last, mode, info=None):
    """One segment's deflate bytes (byte-aligned at both ends)."""
    seg = np.asarray(seg, np.uint8)
    n = len(seg)
    if mode == STORED:
        return stored_segment(seg, last)
    lit, mpos, mlen = tokens(seg)
    len_sym = np.searchsorted(np.array(LEN_BASE), mlen, side="right") - 1
    hist = np.bincount(np.concatenate([seg[lit].astype(np.int64), 257 + len_sym, [256]]), minlength=286).tolist()
    ll, limited = code_lengths(hist, 15)
    llc = canonical(ll)
    hlit = max(s for s in range(286) if ll[s]) + 1                # at least 257: the end-of-block symbol is always used
    seq = length_sequence(ll[:hlit] + [1])                         # one distance code, symbol 0, length 1, match or no match
    clh = [0] * 19
    for s, _, _ in seq:
        clh[s] += 1
    cl, _ = code_lengths(clh, 7)
    clc = canonical(cl)
    hclen = max(i for i in range(19) if cl[CL_ORDER[i]]) + 1
    hclen = max(hclen, 4)
    vals, nb = [1 if last else 0, 2, hlit - 257, 0, hclen - 4], [1, 2, 5, 5, 4]
    for i in range(hclen):
        vals.append(cl[CL_ORDER[i]])
        nb.append(3)
    for s, ev, eb in seq:
        vals.append(clc[s] | ev << cl[s])
        nb.append(cl[s] + eb)
    # the tokens in stream order
    pos = np.concatenate([lit, mpos])
    order = np.argsort(pos, kind="stable")
    llc_a, ll_a = np.array(llc, np.int64), np.array(ll, np.int64)
    lv, lb = llc_a[seg[lit]], ll_a[seg[lit]]
    ms = 257 + len_sym
    eb = np.array(LEN_EXTRA, np.int64)[len_sym]
    mv = llc_a[ms] | (mlen - np.array(LEN_BASE, np.int64)[len_sym]) << ll_a[ms]     # the distance code 0 follows as a 0 bit
    mb = ll_a[ms] + eb + 1
    tv, tb = np.concatenate([lv, mv])[order], np.concatenate([lb, mb])[order]
    vals = np.concatenate([np.array(vals, np.int64), tv, [llc[256]]])
    nb = np.concatenate([np.array(nb, np.int64), tb, [ll[256]]])
    body, bits = _pack(vals, nb)
    if not last:                                                 # the empty stored block: 000, padding, 00 00 FF FF
        body += b"\0" * ((bits + 3 + 7) // 8 - len(body)) + b"\x00\x00\xff\xff"
    if len(body) >= 5 + n:
        if info is not None:
            info["stored_segments"] += 1
        return stored_segment(seg, last)
    if info is not None:
        info["limited_segments"] += int(limited)
        info["matches"] += len(mpos)
    return body


# ---- the file --------------------------------------------------------------------------------------------------------------
def chunk(kind, data):
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data))


def deflate_stream(stream, mode, info=None):
    """The filtered stream -> the zlib stream: header, the segments, the Adler-32."""
    stream = np.asarray(stream, np.uint8)
    nseg = -(-len(stream) // SEGMENT)
    parts = [encode_segment(stream[s * SEGMENT:(s + 1) * SEGMENT], s == nseg - 1, mode, info) for s in range(nseg)]
    return ZLIB_HEADER + b"".join(parts) + struct.pack(">I", zlib.adler32(stream.tobytes()))


def encode(px, filt=ADAPTIVE, mode=RLE, info=None):
    """u8[H,W,3] RGB -> the file's bytes.  `info` (a dict) receives the filtered stream, the row filters and how many segments
    took the stored fallback / had their lengths limited."""
    px = np.ascontiguousarray(px, np.uint8)
    H, W, _ = px.shape
    assert 1 <= H <= MAX_SIDE and 1 <= W <= MAX_SIDE and 0 <= filt <= 5 and mode in (STORED, RLE)
    stream, types = filter_rows(px, 0 if mode == STORED else filt)
    if info is not None:
        info.update(filtered=stream, filters=types, stored_segments=0, limited_segments=0, matches=0,
                    segments=-(-len(stream) // SEGMENT))
    z = deflate_stream(stream, mode, info)
    ihdr = struct.pack(">IIBBBBB", W, H, 8, 2, 0, 0, 0)
    return SIGNATURE + chunk(b"IHDR", ihdr) + chunk(b"IDAT", z) + chunk(b"IEND", b"")


def idat_payload(blob):
    """The concatenated IDAT data of a file and a check of every chunk's CRC -> (zlib stream, chunk kinds)."""
    assert blob[:8] == SIGNATURE
    at, z, kinds = 8, b"", []
    while at < len(blob):
        n, = struct.unpack(">I", blob[at:at + 4])
        kind, data = blob[at + 4:at + 8], blob[at + 8:at + 8 + n]
        crc, = struct.unpack(">I", blob[at + 8 + n:at + 12 + n])
        assert crc == zlib.crc32(kind + data), f"chunk {kind!r}: CRC-32"
        kinds.append(kind)
        if kind == b"IDAT":
            z += data
        at += 12 + n
    assert at == len(blob)
    return z, kinds
