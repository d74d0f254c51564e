"""Section j1b of include/poserisk_hip.h (pr_jpeg_parse_scans, pr_jpeg_decode_scans) restated in plain Python: the scan-aware
marker parser with its refusals and levels, the five entropy procedures of a multi-scan file (sequential scan of a component
subset, DC first, DC refine, AC first, AC refine: ITU-T T.81 annex G) writing coefficients in jpeg_ref.coefficients' layout, and
behind them jpeg_ref's back end, imported and not edited.  Written from the contract and the standard, not from the kernels.

`rescan(stream, script, ...)` is a LOSSLESS TRANSCODER: the coefficients of a baseline stream re-encoded under any scan script
(progressive, or sequential in several scans), with or without restart intervals, with the standard Huffman tables or tables
optimised per scan.  A transcoded stream's pixels are its source's: tests/golden/make_jpeg_progressive_golden.py has Pillow
confirm that for every stream the tests use and stores each stream's SHA-256."""
import numpy as np

import jpeg_enc_ref as er
import jpeg_ref as jr
from jpeg_ref import BadStream, Refused, ZIGZAG, _need

SCAN_BAND, SCAN_AC_COMPONENTS, SCAN_FIRST_AH, SCAN_REFINE, SCAN_AC_BEFORE_DC, SCAN_REFINE_UNSENT, SCAN_TWICE, SCAN_INCOMPLETE = \
    range(16, 24)
MAX_LEVELS = 16

# libjpeg's default progression (jcparam.c, jpeg_simple_progression): (components, Ss, Se, Ah, Al)
LIBJPEG_COLOUR = [((0, 1, 2), 0, 0, 0, 1), ((0,), 1, 5, 0, 2), ((2,), 1, 63, 0, 1), ((1,), 1, 63, 0, 1), ((0,), 6, 63, 0, 2),
                  ((0,), 1, 63, 2, 1), ((0, 1, 2), 0, 0, 1, 0), ((2,), 1, 63, 1, 0), ((1,), 1, 63, 1, 0), ((0,), 1, 63, 1, 0)]
LIBJPEG_GRAY = [((0,), 0, 0, 0, 1), ((0,), 1, 5, 0, 2), ((0,), 6, 63, 0, 2), ((0,), 1, 63, 2, 1), ((0,), 0, 0, 1, 0),
                ((0,), 1, 63, 1, 0)]


def scan_mcus(p, comps):
    """MCUs of a scan of the components `comps` (indices into the frame's) -> (MCUs across, MCUs down, [(c, dy, dx)] the blocks
    of one MCU relative to the MCU's first block of that component, (h, v) per entry's component)."""
    mx, my, _ = jr.geometry(p)
    if len(comps) == 1 and p["ncomp"] == 3:           # one component of three: the blocks of its own size, one a MCU
        c = comps[0]
        dw, dh = (p["width"], p["height"]) if c == 0 else (-(-p["width"] // p["hs"]), -(-p["height"] // p["vs"]))
        return -(-dw // 8), -(-dh // 8), [(c, 0, 0, 1, 1)]
    blocks = []
    for c in comps:
        hc, vc = (p["hs"], p["vs"]) if c == 0 else (1, 1)
        blocks += [(c, b // hc, b % hc, hc, vc) for b in range(hc * vc)]
    return mx, my, blocks


def parse(data):
    """bytes -> dict(width, height, ncomp, hs, vs, progressive, quant u16[ncomp,64] (latched at each component's first scan),
    scans [dict(comps, dc_sel, ac_sel, ss, se, ah, al, restart, level, n_mcus, huff {(class, id): (bits, vals)} of the tables
    the scan uses, segments [(begin, end, first MCU of the scan)])]); raises Refused with pr_jpeg_parse_scans' code."""
    d = bytes(data)
    n = len(d)
    _need(n >= 2 and d[0] == 0xFF and d[1] == 0xD8, jr.NOT_JPEG)
    pos = 2
    qt, huff, sof, restart, scans = {}, {}, None, 0, []
    al_of = level_of = quant = None
    while True:
        _need(pos + 2 <= n, jr.TRUNCATED)
        _need(d[pos] == 0xFF, jr.MARKER)
        m = d[pos + 1]
        pos += 2
        while m == 0xFF:
            _need(pos < n, jr.TRUNCATED)
            m = d[pos]
            pos += 1
        if m == 0xD9:
            _need(scans, jr.SCANS)
            break
        _need(not (m in (0, 1) or 0xD0 <= m <= 0xD8), jr.MARKER)
        _need(pos + 2 <= n, jr.TRUNCATED)
        ln = d[pos] << 8 | d[pos + 1]
        _need(ln >= 2, jr.MARKER)
        _need(pos + ln <= n, jr.TRUNCATED)
        seg = d[pos + 2:pos + ln]
        pos += ln
        _need(m not in (0xC9, 0xCA, 0xCB, 0xCC, 0xCD, 0xCE, 0xCF), jr.ARITHMETIC)
        _need(m not in (0xC1, 0xC3, 0xC5, 0xC6, 0xC7, 0xC8, 0xDC, 0xDE, 0xDF), jr.EXTENDED)
        if m in (0xC0, 0xC2):
            _need(sof is None and len(seg) >= 6, jr.MARKER)
            prec, h, w, nc = seg[0], seg[1] << 8 | seg[2], seg[3] << 8 | seg[4], seg[5]
            _need(prec == 8, jr.PRECISION)
            _need(nc in (1, 3), jr.COMPONENTS)
            _need(16 <= h <= 4096 and 16 <= w <= 4096, jr.DIMENSIONS)
            _need(len(seg) == 6 + 3 * nc, jr.MARKER)
            comps = []
            for c in range(nc):
                cid, hv, tq = seg[6 + 3 * c:9 + 3 * c]
                _need(1 <= hv >> 4 <= 4 and 1 <= hv & 15 <= 4, jr.SAMPLING)
                _need(tq <= 3, jr.TABLE)
                _need(all(cid != o[0] for o in comps), jr.MARKER)
                comps.append((cid, hv >> 4, hv & 15, tq))
            if nc == 3:
                _need((comps[0][1], comps[0][2]) in ((1, 1), (2, 1), (2, 2)), jr.SAMPLING)
                _need(all(c[1] == 1 and c[2] == 1 for c in comps[1:]), jr.SAMPLING)
            sof = dict(width=w, height=h, ncomp=nc, hs=comps[0][1] if nc == 3 else 1, vs=comps[0][2] if nc == 3 else 1,
                       progressive=m == 0xC2)
            al_of, level_of, quant = np.full((nc, 64), -1), np.full((nc, 64), -1), [None] * nc
        elif m == 0xDB:
            p = 0
            while p < len(seg):
                pq = seg[p]
                _need(pq >> 4 != 1, jr.QUANT16)
                _need(pq >> 4 == 0 and pq & 15 <= 3, jr.TABLE)
                _need(p + 65 <= len(seg), jr.MARKER)
                t = np.zeros(64, np.uint16)
                t[ZIGZAG] = np.frombuffer(seg[p + 1:p + 65], np.uint8)
                qt[pq & 15] = t
                p += 65
        elif m == 0xC4:
            p = 0
            while p < len(seg):
                tc = seg[p]
                _need(tc >> 4 <= 1 and tc & 15 <= 1, jr.TABLE)
                _need(p + 17 <= len(seg), jr.MARKER)
                bits = list(seg[p + 1:p + 17])
                _need(sum(bits) <= 256 and p + 17 + sum(bits) <= len(seg), jr.TABLE)
                vals = list(seg[p + 17:p + 17 + sum(bits)])
                _need(tc >> 4 == 1 or all(v <= 15 for v in vals), jr.TABLE)
                huff[(tc >> 4, tc & 15)] = (bits, vals)
                p += 17 + sum(bits)
        elif m == 0xDD:
            _need(len(seg) == 2, jr.MARKER)
            restart = seg[0] << 8 | seg[1]
        elif m == 0xDA:
            _need(sof is not None and len(seg) >= 1, jr.MARKER)
            ns = seg[0]
            _need(1 <= ns <= sof["ncomp"], jr.SCANS)
            _need(len(seg) == 1 + 2 * ns + 3, jr.MARKER)
            ids = [c[0] for c in comps]
            sc = dict(comps=[], dc_sel=[], ac_sel=[])
            for i in range(ns):
                cid, sel = seg[1 + 2 * i], seg[2 + 2 * i]
                _need(cid in ids and (not sc["comps"] or ids.index(cid) > sc["comps"][-1]), jr.SCANS)
                _need(sel >> 4 <= 1 and sel & 15 <= 1, jr.TABLE)
                sc["comps"].append(ids.index(cid))
                sc["dc_sel"].append(sel >> 4)
                sc["ac_sel"].append(sel & 15)
            ss, se, ah, al = seg[1 + 2 * ns], seg[2 + 2 * ns], seg[3 + 2 * ns] >> 4, seg[3 + 2 * ns] & 15
            if not sof["progressive"]:
                _need((ss, se, ah, al) == (0, 63, 0, 0), jr.PROGRESSIVE)
            else:
                _need(ss <= se <= 63 and ah <= 13 and al <= 13 and not (ss == 0 and se != 0), SCAN_BAND)
                _need(ss == 0 or ns == 1, SCAN_AC_COMPONENTS)
                _need(ah == 0 or al == ah - 1, SCAN_REFINE)
            needs_dc, needs_ac = ss == 0 and ah == 0, se > 0
            used, level = {}, 0
            for i, c in enumerate(sc["comps"]):
                _need(ss == 0 or al_of[c, 0] >= 0, SCAN_AC_BEFORE_DC)
                band = al_of[c, ss:se + 1]
                sent = int((band >= 0).sum())
                if ah == 0:
                    _need(sent == 0, SCAN_TWICE)
                else:
                    _need(sent > 0, SCAN_FIRST_AH)
                    _need(sent == len(band), SCAN_REFINE_UNSENT)
                    for v in band:
                        _need(v != al, SCAN_TWICE)
                        _need(v == ah, SCAN_REFINE)
                level = max(level, int(level_of[c, ss:se + 1].max()) + 1)
                al_of[c, ss:se + 1] = al
                _need((not needs_dc or (0, sc["dc_sel"][i]) in huff) and (not needs_ac or (1, sc["ac_sel"][i]) in huff), jr.TABLE)
                if needs_dc:
                    used[(0, sc["dc_sel"][i])] = huff[(0, sc["dc_sel"][i])]
                if needs_ac:
                    used[(1, sc["ac_sel"][i])] = huff[(1, sc["ac_sel"][i])]
                if quant[c] is None:
                    _need(comps[c][3] in qt, jr.TABLE)
                    quant[c] = qt[comps[c][3]].copy()
            _need(level < MAX_LEVELS, SCAN_REFINE)
            for c in sc["comps"]:
                level_of[c, ss:se + 1] = level
            across, down, _ = scan_mcus(sof, sc["comps"])
            sc.update(ss=ss, se=se, ah=ah, al=al, restart=restart, level=level, n_mcus=across * down, huff=used)
            want = -(-sc["n_mcus"] // restart) if restart else 1
            segs, begin, closing = [], pos, None
            while pos < n:
                pos = d.find(b"\xff", pos)
                if pos < 0 or pos + 1 >= n:
                    break
                mk = d[pos + 1]
                if mk == 0:
                    pos += 2
                elif mk == 0xFF:
                    pos += 1
                else:
                    _need(len(segs) < want, jr.RESTARTS)
                    segs.append((begin, pos, len(segs) * restart))
                    if 0xD0 <= mk <= 0xD7:
                        _need(restart and mk == 0xD0 + (len(segs) - 1) % 8, jr.RESTARTS)
                        pos += 2
                        begin = pos
                        continue
                    closing = mk
                    break
            _need(closing is not None, jr.TRUNCATED)
            _need(len(segs) == want, jr.RESTARTS)
            sc["segments"] = segs
            scans.append(sc)
    if (al_of != 0).any():
        raise Refused(jr.SCANS if len(scans) == 1 and not sof["progressive"] else SCAN_INCOMPLETE)
    for sc in scans:
        for bits, _ in sc["huff"].values():             # the counts must form a prefix code
            code = 0
            for l in range(16):
                _need(code + bits[l] <= 1 << (l + 1), jr.TABLE)
                code = (code + bits[l]) << 1
    return dict(sof, quant=np.stack(quant), scans=scans)


def parse_status(data):
    try:
        parse(data)
        return jr.OK
    except Refused as e:
        return e.code


def _int16(v):
    if not -32768 <= v <= 32767:
        raise BadStream("a coefficient outside int16")
    return v


def coefficients(data, p=None):
    """Quantised coefficients per component after every scan: list of int32[bh, bw, 64], natural order (jpeg_ref's layout)."""
    d = bytes(data)
    p = p or parse(d)
    _, _, blocks = jr.geometry(p)
    coef = [np.zeros((bh, bw, 64), np.int32) for bw, bh in blocks]
    for sc in p["scans"]:
        tabs = {k: jr._codes(*v) for k, v in sc["huff"].items()}
        across, down, mcu = scan_mcus(p, sc["comps"])
        ss, se, ah, al = sc["ss"], sc["se"], sc["ah"], sc["al"]
        sel = {c: (sc["dc_sel"][i], sc["ac_sel"][i]) for i, c in enumerate(sc["comps"])}
        for begin, end, first in sc["segments"]:
            raw = d[begin:end]
            cut = raw.find(b"\xff\xff")
            raw = raw if cut < 0 else raw[:cut]
            b = jr._Bits(raw.replace(b"\xff\x00", b"\xff"))
            pred = {c: 0 for c in sc["comps"]}
            eobrun = 0
            n = min(sc["restart"], across * down - first) if sc["restart"] else across * down - first

            def eob_run(r, left):
                extra = 0
                for _ in range(r):
                    extra = extra << 1 | b.bit()
                run = (1 << r) + extra
                if run > left:
                    raise BadStream("an EOB run longer than the blocks left in its segment")
                return run
            for i in range(n):
                m = first + i
                for c, dy, dx, hc, vc in mcu:
                    out = coef[c][(m // across) * vc + dy, (m % across) * hc + dx]
                    if ss == 0 and se == 63:                                   # sequential: jpeg_ref's block decode
                        s = b.symbol(tabs[(0, sel[c][0])])
                        if s:
                            pred[c] += b.extend(s)
                        out[0] = _int16(pred[c])
                        k = 1
                        while k < 64:
                            rs = b.symbol(tabs[(1, sel[c][1])])
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
                    elif ss == 0 and ah == 0:                                  # DC first
                        s = b.symbol(tabs[(0, sel[c][0])])
                        if s:
                            pred[c] += b.extend(s)
                        out[0] = _int16(_int16(pred[c]) * (1 << al))
                    elif ss == 0:                                              # DC refine
                        if b.bit():
                            out[0] |= 1 << al
                    elif ah == 0:                                              # AC first
                        if eobrun > 0:
                            eobrun -= 1
                            continue
                        k = ss
                        while k <= se:
                            rs = b.symbol(tabs[(1, sel[c][1])])
                            r, s = rs >> 4, rs & 15
                            if s == 0 and r != 15:
                                eobrun = eob_run(r, n - i) - 1
                                break
                            k += r if s else 16
                            if k > se:
                                raise BadStream("a run that leaves the band")
                            if s:
                                out[ZIGZAG[k]] = _int16(b.extend(s) * (1 << al))
                                k += 1
                    else:                                                      # AC refine (T.81 G.1.2.3)
                        p1 = 1 << al

                        def correct(k):
                            if b.bit():
                                v = int(out[ZIGZAG[k]])
                                if not v & p1:
                                    out[ZIGZAG[k]] = _int16(v + p1 if v >= 0 else v - p1)
                        k = ss
                        if eobrun == 0:
                            while k <= se:
                                rs = b.symbol(tabs[(1, sel[c][1])])
                                r, s = rs >> 4, rs & 15
                                val = 0
                                if s:
                                    if s != 1:
                                        raise BadStream("a refinement symbol of size above 1")
                                    val = p1 if b.bit() else -p1
                                elif r != 15:
                                    eobrun = eob_run(r, n - i)
                                    break
                                while k <= se:
                                    if out[ZIGZAG[k]]:
                                        correct(k)
                                    else:
                                        r -= 1
                                        if r < 0:
                                            break
                                    k += 1
                                if k > se:
                                    raise BadStream("a run that leaves the band")
                                if s:
                                    out[ZIGZAG[k]] = val
                                k += 1
                        if eobrun > 0:
                            while k <= se:
                                if out[ZIGZAG[k]]:
                                    correct(k)
                                k += 1
                            eobrun -= 1
            if b.pos > 8 * len(b.d):
                raise BadStream("the segment's data ends early")
    return coef


def decode_strict(data, p=None, bgr=False):
    """bytes -> u8[H, W, 3]; BadStream for everything the device must report with a non-zero status."""
    p = p or parse(data)
    coef = coefficients(data, p)
    planes = []
    for c, q in enumerate(coef):
        px, ok = jr.idct(q.astype(np.int64) * p["quant"][c].astype(np.int64))
        if not ok.all():
            raise BadStream("a block outside the 32-bit IDCT bound")
        bh, bw = q.shape[:2]
        planes.append(px.transpose(0, 2, 1, 3).reshape(bh * 8, bw * 8))
    H, W = p["height"], p["width"]
    y = planes[0][:H, :W].astype(np.int64)
    if p["ncomp"] == 1:
        rgb = np.stack([y, y, y], -1)
    else:
        cb = jr.upsample(planes[1], p["hs"], p["vs"], H, W) - 128
        cr = jr.upsample(planes[2], p["hs"], p["vs"], H, W) - 128
        rgb = np.stack([y + ((91881 * cr + 32768) >> 16), y + ((-22554 * cb + 32768 - 46802 * cr) >> 16),
                        y + ((116130 * cb + 32768) >> 16)], -1)
    rgb = np.clip(rgb, 0, 255).astype(np.uint8)
    return rgb[..., ::-1].copy() if bgr else rgb


def verdict(stream):
    """'refused', 'bad' (the parser's rules accept it, decoding by the contract fails) or the decoded pixels."""
    try:
        p = parse(stream)
    except Refused:
        return "refused"
    try:
        return decode_strict(stream, p)
    except BadStream:
        return "bad"


# ---- the lossless transcoder -------------------------------------------------------------------------------------------------
def optimal_table(freq):
    """Symbol counts {symbol: n} -> (bits[16], vals): T.81 K.2 as libjpeg's jpeg_gen_optimal_table runs it (code lengths
    limited to 16, no all-ones code)."""
    f = np.zeros(257, np.int64)
    for s, n in freq.items():
        f[s] = n
    f[256] = 1
    codesize, others = np.zeros(257, np.int64), np.full(257, -1)
    while True:
        nz = np.nonzero(f)[0]
        if len(nz) < 2:
            break
        c1 = max(nz, key=lambda i: (-f[i], i))
        rest = nz[nz != c1]
        c2 = max(rest, key=lambda i: (-f[i], i))
        f[c1] += f[c2]
        f[c2] = 0
        for c, last in ((c1, False), (c2, True)):
            codesize[c] += 1
            while others[c] >= 0:
                c = others[c]
                codesize[c] += 1
            if not last:
                others[c] = c2
    bits = np.zeros(33, np.int64)
    for i in range(257):
        if codesize[i]:
            bits[codesize[i]] += 1
    for i in range(32, 16, -1):
        while bits[i] > 0:
            j = i - 2
            while bits[j] == 0:
                j -= 1
            bits[i] -= 2
            bits[i - 1] += 1
            bits[j + 1] += 2
            bits[j] -= 1
    i = 16
    while bits[i] == 0:
        i -= 1
    bits[i] -= 1
    vals = [s for l in range(1, 33) for s in range(256) if codesize[s] == l]
    return [int(b) for b in bits[1:17]], vals


class _Tokens:
    """One restart segment's symbols and raw bits, kept as tokens until the scan's tables are known."""

    def __init__(self):
        self.t = []

    def symbol(self, table, s):
        self.t.append((table, s))

    def bits(self, value, n):
        if n:
            self.t.append((None, value & ((1 << n) - 1), n))


def _magnitude(v):
    n = int(abs(v)).bit_length()
    return n, (v if v >= 0 else v - 1)


def _scan_tokens(coef, p, comps, ss, se, ah, al, restart, tables, eob_max, stats):
    """-> [_Tokens per restart segment]; tables[c] = ((0, dc id), (1, ac id)); stats['eobrun'] = the longest EOB run emitted."""
    across, down, mcu = scan_mcus(p, comps)
    total = across * down
    segments = []
    for first in range(0, total, restart or total):
        tok, pred, eobrun, pending = _Tokens(), {c: 0 for c in comps}, 0, []
        segments.append(tok)

        def flush():
            nonlocal eobrun, pending
            if eobrun:
                stats["eobrun"] = max(stats.get("eobrun", 0), eobrun)
                n = eobrun.bit_length() - 1
                tok.symbol(ac, n << 4)
                tok.bits(eobrun, n)
                eobrun = 0
            for bit in pending:
                tok.bits(bit, 1)
            pending = []
        for m in range(first, min(first + (restart or total), total)):
            for c, dy, dx, hc, vc in mcu:
                blk = coef[c][(m // across) * vc + dy, (m % across) * hc + dx][ZIGZAG].tolist()
                dc, ac = tables[c]
                if ss == 0 and ah == 0:                                        # DC: sequential, or progressive first
                    v = blk[0] >> al
                    n, low = _magnitude(v - pred[c])
                    pred[c] = v
                    tok.symbol(dc, n)
                    tok.bits(low, n)
                elif ss == 0:
                    tok.bits(blk[0] >> al, 1)
                if se == 0:
                    continue
                lo = max(ss, 1)
                if ah == 0:                                                    # AC: sequential, or progressive first
                    r = 0
                    for k in range(lo, se + 1):
                        mag = abs(blk[k]) >> al
                        if mag == 0:
                            r += 1
                            continue
                        flush()
                        while r > 15:
                            tok.symbol(ac, 0xF0)
                            r -= 16
                        n = mag.bit_length()
                        tok.symbol(ac, r << 4 | n)
                        tok.bits(mag if blk[k] > 0 else ~mag, n)
                        r = 0
                    if r:
                        eobrun += 1
                        if eobrun >= eob_max:
                            flush()
                else:                                                          # AC refine
                    mags = [abs(v) >> al for v in blk]
                    last_new = max([k for k in range(lo, se + 1) if mags[k] == 1], default=-1)
                    r, corr = 0, []
                    for k in range(lo, se + 1):
                        if mags[k] == 0:
                            r += 1
                            continue
                        while r > 15 and k <= last_new:
                            flush()
                            tok.symbol(ac, 0xF0)
                            r -= 16
                            for bit in corr:
                                tok.bits(bit, 1)
                            corr = []
                        if mags[k] > 1:
                            corr.append(mags[k] & 1)
                            continue
                        flush()
                        tok.symbol(ac, r << 4 | 1)
                        tok.bits(0 if blk[k] < 0 else 1, 1)
                        for bit in corr:
                            tok.bits(bit, 1)
                        corr, r = [], 0
                    if r or corr:
                        eobrun += 1
                        pending += corr
                        if eobrun >= eob_max or len(pending) > 937:
                            flush()
        flush()
    return segments


def _entropy_bytes(tok, codes):
    acc, n, out = 0, 0, bytearray()
    for t in tok.t:
        if t[0] is None:
            v, k = t[1], t[2]
        else:
            v, k = codes[t[0]][t[1]]
        acc, n = acc << k | v, n + k
        while n >= 8:
            byte = acc >> (n - 8) & 255
            out.append(byte)
            if byte == 255:
                out.append(0)
            n -= 8
        acc &= (1 << n) - 1
    if n:
        byte = (acc << (8 - n) | ((1 << (8 - n)) - 1)) & 255
        out.append(byte)
        if byte == 255:
            out.append(0)
    return bytes(out)


def _codes_of(bits, vals):
    out, code, k = {}, 0, 0
    for l in range(1, 17):
        for _ in range(bits[l - 1]):
            out[vals[k]] = (code, l)
            code += 1
            k += 1
        code <<= 1
    return out


def _segment(marker, payload):
    return bytes([0xFF, marker, (len(payload) + 2) >> 8, (len(payload) + 2) & 255]) + bytes(payload)


def rescan(stream, script, progressive=True, restart=0, optimize=True, stats=None):
    """The baseline stream's coefficients re-encoded under `script` = [(components, Ss, Se, Ah, Al)] as SOF2 (progressive=True)
    or SOF0 (every scan then (comps, 0, 63, 0, 0)).  restart: MCUs of the scan per restart segment, one int for all scans or a
    list with one per scan (a DRI is written wherever it changes).  optimize=True: every scan gets tables optimised for it,
    DEFINED AS TABLE ID 0 in front of it (so id 0 is redefined before every scan) and a progressive scan may emit EOB runs up to 32767;
    optimize=False: the standard tables (ids 0 luma, 1 chroma), defined once, which hold no EOBn symbol: every EOB run is 1.
    stats: a dict that receives 'eobrun', the longest EOB run emitted."""
    p = jr.parse(stream)
    coef = jr.coefficients(stream, p)
    stats = {} if stats is None else stats
    nc = p["ncomp"]
    out = bytearray(b"\xff\xd8")
    tq = [0] + [0 if np.array_equal(p["quant"][c], p["quant"][0]) else 1 for c in range(1, nc)]
    for t in sorted(set(tq)):
        out += _segment(0xDB, bytes([t]) + bytes(int(v) for v in p["quant"][tq.index(t)][ZIGZAG]))
    sof = bytes([8, p["height"] >> 8, p["height"] & 255, p["width"] >> 8, p["width"] & 255, nc])
    for c in range(nc):
        sof += bytes([c + 1, (p["hs"] << 4 | p["vs"]) if c == 0 and nc == 3 else 0x11, tq[c]])
    out += _segment(0xC2 if progressive else 0xC0, sof)
    std = {(0, 0): (er.DC_BITS[0], er.DC_VALS[0]), (0, 1): (er.DC_BITS[1], er.DC_VALS[1]),
           (1, 0): (er.AC_BITS[0], er.AC_VALS[0]), (1, 1): (er.AC_BITS[1], er.AC_VALS[1])}
    if not optimize:
        for (cls, tid), (bits, vals) in std.items():
            out += _segment(0xC4, bytes([cls << 4 | tid]) + bytes(bits) + bytes(vals))
    current = 0
    for i, (comps, ss, se, ah, al) in enumerate(script):
        ri = restart[i] if isinstance(restart, (list, tuple)) else restart
        if ri != current:
            out += _segment(0xDD, bytes([ri >> 8, ri & 255]))
            current = ri
        ids = {c: (0, 0) if optimize else ((0, 0) if c == 0 else (1, 1)) for c in comps}
        tables = {c: ((0, ids[c][0]), (1, ids[c][1])) for c in comps}
        segs = _scan_tokens(coef, p, comps, ss, se, ah, al, ri, tables, 32767 if optimize and progressive else 1, stats)
        if optimize:
            freq = {}
            for tok in segs:
                for t in tok.t:
                    if t[0] is not None:
                        freq.setdefault(t[0], {}).setdefault(t[1], 0)
                        freq[t[0]][t[1]] += 1
            defs = {k: optimal_table(f) for k, f in freq.items()}
            for (cls, tid), (bits, vals) in sorted(defs.items()):
                out += _segment(0xC4, bytes([cls << 4 | tid]) + bytes(bits) + bytes(vals))
        else:
            defs = std
        codes = {k: _codes_of(*v) for k, v in defs.items()}
        sos = bytes([len(comps)])
        for c in comps:
            sos += bytes([c + 1, ids[c][0] << 4 | ids[c][1]])
        out += _segment(0xDA, sos + bytes([ss, se, ah << 4 | al]))
        for k, tok in enumerate(segs):
            if k:
                out += bytes([0xFF, 0xD0 + (k - 1) % 8])
            out += _entropy_bytes(tok, codes)
    return bytes(out + b"\xff\xd9")
