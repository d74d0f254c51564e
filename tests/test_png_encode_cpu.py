"""The PNG encoder's contract (include/poserisk_hip.h, section j5) as tests/png_enc_ref.py restates it, checked without a GPU
against zlib, Pillow and this package's own decoder reference: every file of every case is a valid PNG that decodes to its
pixels, no file exceeds the bound, the stated rules (stored fallback, length limiter, segment layout) act where the cases
were built to make them act, and the RLE files are no larger than zlib's own Z_RLE strategy allows for."""
import io
import struct
import zlib

import numpy as np
import pytest

import png_enc_cases as ec
import png_enc_ref as ref
import png_ref

CASES = ec.cases()


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_every_file_is_a_valid_png_of_its_pixels(case):
    from PIL import Image
    blob, info = ec.reference(case["name"])
    px = case["px"]
    H, W, _ = px.shape
    z, kinds = ref.idat_payload(blob)                            # asserts every chunk's CRC-32 against zlib.crc32
    assert kinds == [b"IHDR", b"IDAT", b"IEND"]
    raw = zlib.decompress(z)
    assert len(raw) == H * (1 + 3 * W) and raw == info["filtered"].tobytes()
    assert struct.unpack(">I", z[-4:])[0] == zlib.adler32(raw)
    st, un = png_ref.unfilter(raw, H, W, 3)
    assert st == 0 and np.array_equal(un.reshape(H, W, 3), px)
    assert np.array_equal(np.asarray(Image.open(io.BytesIO(blob)).convert("RGB")), px)
    pst, dst, got = png_ref.decode(blob)
    assert pst == 0 and dst == 0 and np.array_equal(got, px)
    assert len(blob) <= ref.bound(H, W)
    if case["mode"] == ref.STORED:
        assert len(blob) == ref.bound(H, W) and not info["filters"].any()
    elif case["filter"] < 5:
        assert (info["filters"] == case["filter"]).all()


def _segment_heads(blob, H, W):
    """The first byte of every segment of a file whose segments are all stored blocks (asserted from the sizes)."""
    z, _ = ref.idat_payload(blob)
    raw = H * (1 + 3 * W)
    nseg = -(-raw // ref.SEGMENT)
    assert len(z) == 2 + raw + 5 * nseg + 4, "not every segment is a stored block"
    at, heads = 2, []
    for s in range(nseg):
        n = min(ref.SEGMENT, raw - s * ref.SEGMENT)
        head, ln, nln = struct.unpack("<BHH", z[at:at + 5])
        assert ln == n and nln == n ^ 0xFFFF
        heads.append(head)
        at += 5 + n
    return heads


@pytest.mark.parametrize("name", [c["name"] for c in CASES if "_noise" in c["name"] or c["mode"] == ref.STORED])
def test_noise_and_stored_mode_are_stored_blocks_by_their_bytes(name):
    case = next(c for c in CASES if c["name"] == name)
    blob, info = ec.reference(name)
    H, W, _ = case["px"].shape
    heads = _segment_heads(blob, H, W)
    assert heads == [0] * (len(heads) - 1) + [1]                 # stored, BFINAL on the last one only
    if case["mode"] == ref.RLE:
        assert info["stored_segments"] == info["segments"]


def test_the_special_cases_do_what_they_were_built_for():
    info = {n: ec.reference(n)[1] for n in ("4096x1_runs_f0_rle", "683x9_crossing_f0_rle", "64x40_nomatch_f0_rle",
                                            "3648x1_fibonacci_f0_rle", "1000x1_two_values_f0_rle")}
    # runs of 1, 2, 3 -> literals only; 4 -> one literal and a match of 3; 259 -> literal + 258; 260, 261 -> + 1, 2 literals;
    # 262 -> literal + 258 + 3; 517 -> literal + 258 + 258
    stream = info["4096x1_runs_f0_rle"]["filtered"]
    lit, mpos, mlen = ref.tokens(stream)
    at, want = 1, []
    for n in ec.RUN_LENGTHS:
        rest = n - 1
        while rest >= 3:
            want.append((at + n - rest, min(rest, 258)))
            rest -= min(rest, 258)
        at += n
    assert list(zip(mpos.tolist(), mlen.tolist())) == want and len(want) == 1 + 1 + 1 + 1 + 1 + 2 + 2
    # the crossing run is cut at the boundary: the second segment starts with a literal
    stream = info["683x9_crossing_f0_rle"]["filtered"]
    assert (stream[16251:16400] == 77).all() and stream[16250] != 77
    _, mpos, mlen = ref.tokens(stream[:ref.SEGMENT])
    assert mpos[-1] + mlen[-1] == ref.SEGMENT
    lit, mpos, _ = ref.tokens(stream[ref.SEGMENT:])
    assert lit[0] == 0 and mpos[0] == 1
    assert info["64x40_nomatch_f0_rle"]["matches"] == 0 and info["64x40_nomatch_f0_rle"]["stored_segments"] == 0
    fib = info["3648x1_fibonacci_f0_rle"]
    assert sorted(np.bincount(fib["filtered"])[np.bincount(fib["filtered"]) > 0].tolist()) == sorted(ec.FIBONACCI)
    assert fib["matches"] == 0 and fib["limited_segments"] == 1 and fib["stored_segments"] == 0
    two = info["1000x1_two_values_f0_rle"]
    assert set(two["filtered"].tolist()) == {0, 7} and two["matches"] == 0 and two["stored_segments"] == 0


def test_the_limiter_keeps_a_complete_code_of_at_most_fifteen_bits():
    hist = list(ec.FIBONACCI) + [1]
    lens, limited = ref.code_lengths(hist, 15)
    assert limited and max(lens) == 15 and sum(2 ** (15 - v) for v in lens if v) == 2 ** 15
    free, _ = ref.code_lengths(hist, 32)
    assert max(free) == 19
    for n in range(2, 20):                                       # every small alphabet: complete, within the limit
        lens, _ = ref.code_lengths([1 << i for i in range(n)], 7)
        assert max(lens) <= 7 and sum(2 ** (7 - v) for v in lens if v) == 2 ** 7


def test_adaptive_picks_the_smallest_sum_and_the_lowest_number_on_ties():
    px = ec.smooth(160, 90)
    _, types = ref.filter_rows(px, ref.ADAPTIVE)
    fixed = [ref.filter_rows(px, t)[0].reshape(90, -1)[:, 1:].astype(np.int64) for t in range(5)]
    cost = np.stack([np.where(v < 128, v, 256 - v).sum(1) for v in fixed])
    assert np.array_equal(types, cost.argmin(0))                 # argmin: the first of equal minima
    assert len(set(types.tolist())) > 1
    _, types = ref.filter_rows(np.zeros((4, 7, 3), np.uint8), ref.ADAPTIVE)
    assert not types.any()


# The reference's RLE file against zlib.compressobj(6, DEFLATED, 15, 8, Z_RLE) on the same filtered bytes, both deterministic.
# Measured with zlib 1.2.11: 160x90 smooth 15 979 / 15 914 = 1.0041, 683x9 smooth 6 671 / 6 611 = 1.0091, the 1000x450 canvas
# 447 797 / 446 781 = 1.0023 (the file's 57 bytes of signature and chunks are counted on our side only, which the small cases
# show); the bound is the measured ratio rounded up to the next 0.01.
SIZE_RATIO = {"160x90": 1.01, "683x9": 1.01, "canvas": 1.01}


@pytest.mark.parametrize("which", list(SIZE_RATIO))
def test_rle_file_size_against_zlibs_own_rle_strategy(which):
    px = ec.canvas() if which == "canvas" else ec.smooth(*map(int, which.split("x")))
    info = {}
    blob = ref.encode(px, ref.ADAPTIVE, ref.RLE, info)
    co = zlib.compressobj(6, zlib.DEFLATED, 15, 8, zlib.Z_RLE)
    theirs = co.compress(info["filtered"].tobytes()) + co.flush()
    ratio = len(blob) / len(theirs)
    print(f"{which}: {len(blob)} bytes, zlib Z_RLE {len(theirs)}, ratio {ratio:.4f}")
    assert ratio <= SIZE_RATIO[which]
    assert zlib.decompress(ref.idat_payload(blob)[0]) == info["filtered"].tobytes()


def test_bound_counts_five_bytes_a_segment():
    assert ref.bound(1, 1) == 63 + 4 + 5
    assert ref.bound(64, 85) == 63 + 16384 + 5 and ref.bound(65, 85) == 63 + 16640 + 10
