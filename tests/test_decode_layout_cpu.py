"""The two pure pieces of the decoders' chunk loop (poserisk_release_amd/_media.py::decode_chunks), without a GPU and without
the library: where the descriptor arrays lie behind the files' bytes in the one buffer (`_media.layout`), and how
png.decode_files cuts its files into chunks by count and by `max_bytes` (`png.cut_chunk`).  Both against restatements of
what jpeg.decode_files and png.decode_files computed inline before the loop was shared."""
import numpy as np
import pytest

from poserisk_release_amd import _media, jpeg, png


def _align(n, a=256):
    return (n + a - 1) // a * a


def _cut_inline(sizes, lo, chunk, per_frame, max_bytes):
    """png.decode_files' inner `while`, as it stood in the loop."""
    F = len(sizes)
    n, total = 0, 0
    while lo + n < F and n < chunk and (n == 0 or (n + 1) * per_frame + total + sizes[lo + n] + 32 <= max_bytes):
        total += sizes[lo + n]
        n += 1
    return n


def _walk(cut, sizes, *args):
    out, lo = [], 0
    while lo < len(sizes):
        out.append(cut(sizes, lo, *args))
        assert out[-1] >= 1
        lo += out[-1]
    return out


def test_png_cut_rule_equals_the_inline_loop_on_random_draws():
    rng = np.random.default_rng(2024)
    cut_short = 0
    for _ in range(200):
        F = int(rng.integers(1, 40))
        sizes = [int(v) for v in rng.integers(0, 60000, F)]
        chunk = int(rng.integers(1, 12))
        per_frame = int(rng.integers(0, 120000))
        max_bytes = int(rng.integers(0, 6 * (per_frame + 30000) + 1))
        got = _walk(png.cut_chunk, sizes, chunk, per_frame, max_bytes)
        assert got == _walk(_cut_inline, sizes, chunk, per_frame, max_bytes), (sizes, chunk, per_frame, max_bytes)
        assert sum(got) == F and max(got) <= chunk
        cut_short += any(n < chunk for n in got[:-1])
    assert cut_short > 50                                                    # the draws do reach the byte rule, not only the count


def test_png_cut_rule_at_its_edges():
    # a file larger than max_bytes still forms a chunk of one, and its neighbours are not dragged in
    assert _walk(png.cut_chunk, [10, 10 ** 9, 10, 10], 8, 100, 1000) == [1, 1, 2]
    assert _walk(png.cut_chunk, [10 ** 9], 8, 100, 0) == [1]
    # chunk=1: the byte rule never gets a say
    assert _walk(png.cut_chunk, [5, 5, 5], 1, 0, 1 << 40) == [1, 1, 1]
    # all files empty: per_frame and the 32 bytes alone decide
    assert _walk(png.cut_chunk, [0] * 7, 1024, 100, 3 * 100 + 32) == [3, 3, 1]
    assert _walk(png.cut_chunk, [0] * 7, 1024, 100, 3 * 100 + 31) == [2, 2, 2, 1]
    assert _walk(png.cut_chunk, [0] * 7, 4, 0, 0) == [1] * 7                 # 32 > 0: one a chunk
    assert _walk(png.cut_chunk, [0] * 7, 4, 0, 32) == [4, 3]
    assert png.cut_chunk([], 0, 4, 0, 32) == 0 and png.cut_chunk([1, 2], 2, 4, 0, 32) == 0
    # exactly at the bound and one byte below it
    sizes, per_frame = [1000, 2000, 3000], 500
    assert png.cut_chunk(sizes, 0, 8, per_frame, 3 * per_frame + 6000 + 32) == 3
    assert png.cut_chunk(sizes, 0, 8, per_frame, 3 * per_frame + 6000 + 31) == 2


def test_layout_is_aligned_and_disjoint():
    rng = np.random.default_rng(7)
    for _ in range(200):
        total = int(rng.integers(0, 5000)) * int(rng.integers(0, 2))
        arrays = [(int(rng.integers(1, 3000)), int(rng.integers(0, 40))) for _ in range(int(rng.integers(1, 6)))]
        at, end = _media.layout(total, arrays)
        assert len(at) == len(arrays) and all(o % 256 == 0 for o in at)
        assert at[0] >= max(total, 1)
        for k, (itemsize, count) in enumerate(arrays):
            stop = at[k] + itemsize * count
            assert stop <= (at[k + 1] if k + 1 < len(arrays) else end)
        assert end == at[-1] + arrays[-1][0] * arrays[-1][1]
    assert _media.layout(0, [(8, 3)]) == ([256], 256 + 24)                   # no bytes at all: the first array still behind one
    assert _media.layout(256, [(8, 3)]) == ([256], 256 + 24) and _media.layout(257, [(8, 3)]) == ([512], 512 + 24)


def _jpeg_inline(total, n, seg_room, scan_room, huff_room, progressive):
    """jpeg.decode_files' offsets as it computed them: [file bytes | frames | segments | (segments' scans | scans |) table sets]"""
    o_fr = _align(max(total, 1))
    o_seg = _align(o_fr + n * jpeg.FRAME_DTYPE.itemsize)
    o_ss = _align(o_seg + seg_room * jpeg.SEGMENT_DTYPE.itemsize)
    o_sc = _align(o_ss + (seg_room * 4 if progressive else 0))
    o_huff = _align(o_sc + scan_room * jpeg.SCAN_DTYPE.itemsize)
    return [o_fr, o_seg, o_ss, o_sc, o_huff], o_huff + huff_room * jpeg.HUFF_DTYPE.itemsize


def _png_inline(total, n, pal_room, idat_room):
    """png.decode_files' offsets as it computed them: [file bytes | frames | palettes | IDAT ranges]"""
    o_fr = _align(max(total, 1))
    o_pal = _align(o_fr + n * png.FRAME_DTYPE.itemsize)
    o_idat = _align(o_pal + pal_room * png.PALETTE_BYTES)
    return [o_fr, o_pal, o_idat], o_idat + idat_room * png.IDAT_DTYPE.itemsize


JPEG_SIZES = [jpeg.FRAME_DTYPE.itemsize, jpeg.SEGMENT_DTYPE.itemsize, 4, jpeg.SCAN_DTYPE.itemsize, jpeg.HUFF_DTYPE.itemsize]
PNG_SIZES = [png.FRAME_DTYPE.itemsize, png.PALETTE_BYTES, png.IDAT_DTYPE.itemsize]


@pytest.mark.parametrize("total, n, seg_room, scan_room, huff_room", [(0, 1, 66, 10, 1), (9426, 1, 72, 10, 1), (1234567, 256, 64 + 57 * 256, 2560, 300)])
def test_layout_equals_the_jpeg_order(total, n, seg_room, scan_room, huff_room):
    # baseline: the two arrays in the middle are empty and take no room
    at, end = _media.layout(total, list(zip(JPEG_SIZES, [n, seg_room, 0, 0, huff_room])))
    want, want_end = _jpeg_inline(total, n, seg_room, 0, huff_room, False)
    assert (at, end) == (want, want_end) and at[2] == at[3] == at[4]
    at, end = _media.layout(total, list(zip(JPEG_SIZES, [n, seg_room, seg_room, scan_room, huff_room])))
    assert (at, end) == _jpeg_inline(total, n, seg_room, scan_room, huff_room, True)
    assert at[1] < at[2] < at[3] < at[4] < end


@pytest.mark.parametrize("total, n, idat_room", [(0, 1, 18), (700, 1, 57), (40 << 20, 256, 16 + 640 * 256)])
def test_layout_equals_the_png_order(total, n, idat_room):
    at, end = _media.layout(total, list(zip(PNG_SIZES, [n, n, idat_room])))
    assert (at, end) == _png_inline(total, n, n, idat_room)
    assert at[0] < at[1] < at[2] < end
