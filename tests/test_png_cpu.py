"""The PNG decoder without a GPU: the reference model (tests/png_ref.py) against its oracles -- Pillow's .convert("RGB") for the
pixels, zlib.decompress for the inflate, on every case and on the bad-stream list -- and pr_png_parse through the built library
against the reference's chunk walk: descriptors, ranges, every refusal by name, the capacity protocol."""
import io
import struct
import zlib

import numpy as np
import pytest

import png_cases as pc
import png_ref as ref
from poserisk_release_amd import _lib, jpeg, png


def _pillow_rgb(blob):
    from PIL import Image                                                       # the pixel oracle: without it these tests fail
    return np.asarray(Image.open(io.BytesIO(blob)).convert("RGB"))


def test_the_reference_equals_pillow_and_zlib_on_every_case():
    cases = pc.small_cases()
    assert len(cases) >= 170
    for name, blob, want in cases:
        pst, st, px, info = ref.decode(blob, want_info=True)
        assert (pst, st) == (0, 0), name
        assert np.array_equal(px, want), name                                  # what the case was made from
        assert np.array_equal(px, _pillow_rgb(blob)), name                     # what Pillow reads
        assert np.array_equal(ref.decode(blob, bgr=True)[2], want[..., ::-1]), name
        fr = ref.parse(blob)
        z = b"".join(blob[b:e] for b, e in fr["idat"])
        assert ref.inflate(z)[1] == zlib.decompress(z), name


def test_a_palette_index_past_plte_reads_black_as_in_pillow():
    raw = b"\0" + bytes([0, 1, 2, 3, 200])
    blob = pc.png(5, 1, 3, zlib.compress(raw), palette=bytes([10, 20, 30, 40, 50, 60, 70, 80, 90]))
    px = ref.decode(blob)[2]
    assert px.tolist() == [[[10, 20, 30], [40, 50, 60], [70, 80, 90], [0, 0, 0], [0, 0, 0]]]
    assert np.array_equal(px, _pillow_rgb(blob))


def test_the_large_frames_are_what_pillow_reads():
    for name, blob, want in pc.large_frames():
        assert np.array_equal(_pillow_rgb(blob), want), name
        fr = ref.parse(blob)
        assert fr["status"] == 0 and (len(fr["idat"]) > 1 or "stored" in name), name


def test_the_reference_flags_exactly_the_streams_zlib_rejects():
    """Every single-byte XOR of one small dynamic stream and its truncation at every offset (the bad-stream list the native and
    GPU tests draw from), then 2000 seeded corruptions: the reference's status is non-zero exactly where zlib.decompress
    raises or the length differs, and where both accept the bytes are equal."""
    z, nraw = pc.fuzz_base()
    streams = pc.xor_mutations(z) + pc.truncations(z) + pc.corruptions(z)
    assert len(streams) == 2 * len(z) + 2000
    accepted = 0
    for i, s in enumerate(streams):
        want = ref.zlib_verdict(s, nraw)
        if len(s) >= 2 and (s[0] & 15 != 8 or s[0] >> 4 > 7 or s[1] & 32 or (s[0] * 256 + s[1]) % 31):
            assert want is None and ref.parse(pc.wrap(s))["status"] == ref.E_ZLIB_HEADER, i   # the parser's part of the rule
            continue
        st, out, adler, _ = ref.inflate(s, nraw)
        if st == 0 and ref.adler32(out) != adler:
            st = ref.ST_CHECKSUM
        assert (st != 0) == (want is None), (i, st)
        if want is not None:
            accepted += 1
            assert out == want, i
    assert 1 <= accepted < 40, accepted                                        # both classes occur


def test_the_gpu_bad_files_carry_the_status_bit_they_are_named_for():
    for name, blob, bit in pc.gpu_bad_files():
        pst, st, _ = ref.decode(blob)
        assert st == bit and (pst != 0) == (bit == ref.ST_REFUSED), (name, pst, st)
        if pst == 0:
            fr = ref.parse(blob)
            z = b"".join(blob[b:e] for b, e in fr["idat"])
            ok = ref.zlib_verdict(z, fr["height"] * (1 + fr["width"] * fr["bpp"])) is not None
            assert ok == (bit == ref.ST_FILTER), name                           # zlib knows nothing of filter bytes


# ---- pr_png_parse through the built library --------------------------------------------------------------------------------
def test_abi_version_is_still_16():
    assert _lib.load().pr_abi_version() == 16 == _lib.ABI_VERSION


def test_parse_gives_the_references_descriptors_and_ranges_on_every_case():
    for (W, H), cases in pc.by_size().items():
        blobs = [b for _, b, _ in cases]
        frames, idat, palettes, pst, h, w, offsets = png.parse(blobs)
        assert (h, w) == (H, W) and not pst.any()
        n_pal = 0
        for k, ((name, blob, _), fr) in enumerate(zip(cases, frames)):
            want = ref.parse(blob)
            assert (fr["width"], fr["height"], fr["color_type"], fr["bpp"], fr["zlib_bytes"]) == \
                (want["width"], want["height"], want["color_type"], want["bpp"], want["zlib_bytes"]), name
            mine = idat[fr["first_idat"]:fr["first_idat"] + fr["n_idat"]]
            assert [(int(g["begin"] - offsets[k]), int(g["end"] - offsets[k])) for g in mine] == want["idat"], name
            if want["palette"] is None:
                assert fr["palette"] == -1, name
            else:
                assert fr["palette"] == n_pal and palettes[n_pal].tobytes() == want["palette"], name
                n_pal += 1
        assert len(palettes) == n_pal and len(idat) == sum(int(f["n_idat"]) for f in frames)


def _rechunk(blob, edit):
    """The file with its chunk list [(type, body)] passed through `edit` and written back with right CRCs."""
    chunks, p = [], 8
    while p < len(blob):
        ln, = struct.unpack(">I", blob[p:p + 4])
        chunks.append((blob[p + 4:p + 8], blob[p + 8:p + 8 + ln]))
        p += 12 + ln
    return ref.SIGNATURE + b"".join(pc.chunk(t, b) for t, b in edit(chunks))


def _ihdr(**kw):
    def edit(chunks):
        f = dict(zip(("w", "h", "depth", "ct", "comp", "filt", "lace"), struct.unpack(">IIBBBBB", chunks[0][1])))
        f.update(kw)
        return [(b"IHDR", struct.pack(">IIBBBBB", *f.values()))] + chunks[1:]
    return edit


def _zhead(a, b):
    return lambda chunks: [(t, bytes([a, b]) + body[2:]) if t == b"IDAT" else (t, body) for t, body in chunks]


def test_every_refusal_fires_by_name_on_a_minimal_mutation():
    good = next(b for n, b, _ in pc.small_cases() if n.startswith("5x3 ct2 filter0"))
    pal = next(b for n, b, _ in pc.small_cases() if n.startswith("5x3 ct3 filter0"))
    crc = bytearray(good)
    crc[-5] ^= 1                                                             # IEND's CRC
    mutations = {
        ref.E_SIGNATURE: [b"\x89PNX" + good[4:], b"", good[:7]],
        ref.E_TRUNCATED: [good[:-1], good[:20], good[:8]],
        ref.E_CRC: [bytes(crc), good[:30] + bytes([good[30] ^ 8]) + good[31:]],
        ref.E_CHUNK_ORDER: [_rechunk(good, lambda c: c[1:]), _rechunk(good, lambda c: [c[0], c[0]] + c[1:]),
                            _rechunk(good, lambda c: [c[0], c[-1]]), _rechunk(pal, lambda c: [x for x in c if x[0] != b"PLTE"]),
                            _rechunk(pal, lambda c: [c[0], c[2], c[1], c[3]]), _rechunk(good, lambda c: [c[0], c[1], (b"tEXt", b"a\0b"), c[1], c[2]]),
                            _rechunk(good, lambda c: [c[0], (b"PLTE", bytes(4))] + c[1:]), _rechunk(good, lambda c: [(b"IHDR", c[0][1] + b"\0")] + c[1:]),
                            _rechunk(good, lambda c: c[:-1] + [(b"IEND", b"x")]), _rechunk(good, lambda c: [(b"tEXt", b"a\0b")] + c)],
        ref.E_DEPTH16: [_rechunk(good, _ihdr(depth=16))],
        ref.E_DEPTH_SUB8: [_rechunk(pal, _ihdr(depth=d)) for d in (1, 2, 4)] + [_rechunk(good, _ihdr(depth=4, ct=0))],
        ref.E_INTERLACE: [_rechunk(good, _ihdr(lace=1))],
        ref.E_CGBI: [_rechunk(good, lambda c: [(b"CgBI", bytes(4))] + c)],
        ref.E_IHDR: [_rechunk(good, _ihdr(ct=5)), _rechunk(good, _ihdr(depth=3)), _rechunk(good, _ihdr(depth=4)), _rechunk(good, _ihdr(comp=1)),
                     _rechunk(good, _ihdr(filt=1)), _rechunk(good, _ihdr(lace=2)), _rechunk(good, _ihdr(w=0)), _rechunk(good, _ihdr(h=4097)),
                     _rechunk(pal, _ihdr(depth=16))],
        ref.E_ZLIB_HEADER: [_rechunk(good, _zhead(0x79, 0x9c)), _rechunk(good, _zhead(0x88, 0x1c)), _rechunk(good, _zhead(0x78, 0xbb)),
                            _rechunk(good, _zhead(0x78, 0x9d)), _rechunk(good, lambda c: [c[0], (b"IDAT", b"\x78"), c[-1]])],
    }
    assert set(mutations) | {ref.E_OK, ref.E_SIZE_DIFFERS} == set(range(12))
    names = set()
    for code, blobs in mutations.items():
        for i, blob in enumerate(blobs):
            assert ref.parse(blob)["status"] == code, (code, i, ref.parse(blob)["status"])
            frames, idat, _, pst, h, w, _ = png.parse([good, blob, good])
            assert pst.tolist() == [0, code, 0] and (h, w) == (3, 5), (code, i, pst.tolist())
            assert frames[1]["bpp"] == 0 and frames[1]["n_idat"] == 0 and len(idat) == 2
            assert zlib_agrees(blob, code)
        names.add(png.refusal_name(code))
    assert len(names) == len(mutations) and all(names)
    # a size other than the call's, by the first accepted frame and by the caller's H, W
    other = next(b for n, b, _ in pc.small_cases() if n.startswith("7x1 ct2 filter0"))
    assert png.parse([good, other])[3].tolist() == [0, ref.E_SIZE_DIFFERS]
    assert png.parse([other, good])[3].tolist() == [0, ref.E_SIZE_DIFFERS]
    assert png.parse([good], H=1, W=7)[3].tolist() == [ref.E_SIZE_DIFFERS] and ref.parse(good, 1, 7)["status"] == ref.E_SIZE_DIFFERS
    assert "size differs" in png.refusal_name(ref.E_SIZE_DIFFERS) and png.refusal_name(99) == "unknown refusal code"


def zlib_agrees(blob, code):
    """A zlib-header refusal is one zlib.decompress raises on too."""
    if code != ref.E_ZLIB_HEADER:
        return True
    p, z = 8, b""
    while p < len(blob):
        ln, = struct.unpack(">I", blob[p:p + 4])
        if blob[p + 4:p + 8] == b"IDAT":
            z += blob[p + 8:p + 8 + ln]
        p += 12 + ln
    try:
        zlib.decompress(z)
    except zlib.error:
        return True
    return False


def test_the_capacity_protocol_reports_what_is_needed():
    import ctypes as C
    cases = pc.by_size()[(33, 17)]
    blobs = [b for _, b, _ in cases]
    frames, idat, palettes, pst, H, W, offsets = png.parse(blobs)
    assert len(idat) > 100                                                    # the 1-byte IDATs
    data = np.frombuffer(b"".join(blobs), np.uint8)
    fr, st = np.zeros(len(blobs), png.FRAME_DTYPE), np.zeros(len(blobs), np.int32)
    small, nopal = np.zeros(3, png.IDAT_DTYPE), np.zeros(0, np.uint8)
    rc, counts = png._parse_into(data, offsets, 0, 0, fr, small, nopal, st)
    assert rc == -4 and counts.tolist() == [len(idat), len(palettes), 17, 33]
    assert "ranges" in _lib.load().pr_last_error().decode()
    exact, pal = np.zeros(len(idat), png.IDAT_DTYPE), np.zeros(len(palettes) * 768, np.uint8)
    rc, counts = png._parse_into(data, offsets, 0, 0, fr, exact, pal, st)
    assert rc == 0 and np.array_equal(exact, idat) and np.array_equal(fr, frames)
    lib = _lib.load()
    assert lib.pr_png_parse(None, None, 0, 0, 0, None, None, 0, None, 0, None, counts.ctypes.data_as(C.c_void_p)) == 0      # F = 0
    assert lib.pr_png_parse(None, None, 1, 0, 0, None, None, 0, None, 0, None, counts.ctypes.data_as(C.c_void_p)) == -1
    assert lib.pr_png_parse(None, None, 0, 5000, 5, None, None, 0, None, 0, None, counts.ctypes.data_as(C.c_void_p)) == -1


def test_workspace_bytes_and_the_words():
    assert png.workspace_bytes(0, 4, 4, 10) == 0 and png.workspace_bytes(1, 4097, 4, 10) == 0 and png.workspace_bytes(1, 4, 4, -1) == 0
    one, two = png.workspace_bytes(1, 450, 800, 1000), png.workspace_bytes(2, 450, 800, 1000)
    assert one % 16 == 0 and two - one >= 450 * (1 + 4 * 800) and one >= 1000 + 450 * (1 + 4 * 800)
    assert png.status_text(0) == "ok" and all(png.status_text(1 << b) != "ok" for b in range(6))
    assert len({png.status_text(1 << b) for b in range(6)}) == 6
    assert (png.ST_REFUSED, png.ST_TRUNCATED, png.ST_BAD_CODE, png.ST_SIZE, png.ST_FILTER, png.ST_CHECKSUM) == \
        (ref.ST_REFUSED, ref.ST_TRUNCATED, ref.ST_BAD_CODE, ref.ST_SIZE, ref.ST_FILTER, ref.ST_CHECKSUM)


def test_list_frames_orders_png_names_and_jpeg_still_refuses_them(tmp_path):
    for n in ("000000010.png", "000000002.PNG", "000000001.png", "tracking.pkl", "fps.txt", "b.jpg.txt", "thumb.pngx"):
        (tmp_path / n).write_bytes(b"")
    assert png.list_frames(str(tmp_path)) == ["000000001.png", "000000002.PNG", "000000010.png"]
    with pytest.raises(ValueError, match="PNG"):
        jpeg.list_frames(str(tmp_path))
    (tmp_path / "000000003.jpg").write_bytes(b"")
    assert png.list_frames(str(tmp_path)) == ["000000001.png", "000000002.PNG", "000000010.png"]   # the caller refuses the mix
    with pytest.raises(ValueError, match="PNG"):
        jpeg.list_frames(str(tmp_path))


def test_decode_files_has_no_cpu_fallback():
    with pytest.raises(_lib.PoseRiskHipError, match="GPU only"):
        png.decode_files([], "cpu")
