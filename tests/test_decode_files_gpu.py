"""What `jpeg.decode_files` and `png.decode_files` promise about their chunks, through the public calls only: the chunk size is
invisible in frames, status and `bad_frames`; a call whose size arrives in a later chunk; a call that accepts nothing; a chunk
behind the first whose descriptors outgrow the first guess, and (JPEG at 80 wide, PNG) with them the pinned buffer; `out`
checked before anything is written; PNG's cut by `max_bytes`.  Every picture is at most 160 x 90.  No test provokes a fault:
the bad items are refused by the host parser or flagged by a status bit, as tests/test_jpeg_gpu.py and tests/test_png_gpu.py
already have them."""
import functools

import numpy as np
import pytest
import torch

import jpeg_cases as jc
import jpeg_enc_ref as er
import jpeg_ref as jr
import jpeg_scans_cases as sc
import png_cases as pc
from poserisk_release_amd import _lib, _media, jpeg, png

pytestmark = pytest.mark.gpu

FORMATS = [pytest.param(jpeg, {}, id="jpeg"), pytest.param(jpeg, {"progressive": True}, id="jpeg-progressive"),
           pytest.param(png, {}, id="png")]
GARBAGE = [bytes([k]) + b"garbage: neither a JPEG nor a PNG file\xff" * (k + 2) for k in range(3)]   # the host parsers refuse these


@functools.lru_cache(maxsize=None)
def _same_size(module):
    """(five good (file, pixels) of one size, a truncated stream of that size)"""
    if module is jpeg:
        good = [(s, px) for n, s, px in jc.small_cases() if n.startswith("33x17")][:5]
        cut = jc.fuzz_base()                                                 # 33x17 too; every truncation is proven on the host
        return good, cut[:len(cut) * 2 // 3]
    good = [(s, px) for _, s, px in pc.by_size()[(160, 90)]][:5]
    name, cut, bit = pc.gpu_bad_files()[1]
    assert bit == png.ST_TRUNCATED
    return good, cut


def _seven(module):
    """Seven items of one size -> (items, expected pixels or None): garbage at 2, the truncated stream at 5."""
    good, cut = _same_size(module)
    items = [good[0][0], good[1][0], GARBAGE[0], good[2][0], good[3][0], cut, good[4][0]]
    want = [good[0][1], good[1][1], None, good[2][1], good[3][1], None, good[4][1]]
    return items, want


def _late_goods(module, kw):
    """Two good (file, pixels) of one size; with progressive=True files in several scans, so that the chunks take that entry."""
    if kw.get("progressive"):
        return [(s, px) for _, s, px in sc.all_small() if px.shape[:2] == (17, 33)][:2]
    return list(_same_size(module)[0][:2])


@pytest.mark.parametrize("module, kw", FORMATS)
def test_the_chunk_size_is_invisible(gpu_device, module, kw):
    items, want = _seven(module)
    whole = None
    for chunk in (7, 1, 2, 3):
        frames, status = module.decode_files(items, gpu_device, chunk=chunk, **kw)
        words = module.bad_frames(items, status, **kw)
        got, st = frames.cpu().numpy(), status.cpu().numpy()
        if whole is None:
            whole = (got, st, words)
            assert got.shape == (7,) + want[0].shape and got.dtype == np.uint8 and st.dtype == np.int32
            for k, px in enumerate(want):
                if px is None:
                    assert st[k] != 0, f"bad item {k} came back with status 0"
                else:
                    assert st[k] == 0 and np.array_equal(got[k], px), f"good frame {k}: status {st[k]}"
            assert st[2] & module.ST_REFUSED and not got[2].any()
            assert [i for i, _ in words] == [2, 5] and all(w for _, w in words)
        assert got.tobytes() == whole[0].tobytes() and st.tobytes() == whole[1].tobytes(), f"chunk={chunk} differs from chunk=7"
        assert words == whole[2], f"chunk={chunk}: {words} for {whole[2]}"


@pytest.mark.parametrize("module, kw", FORMATS)
def test_the_size_arrives_in_a_later_chunk(gpu_device, module, kw):
    good = _late_goods(module, kw)
    items = GARBAGE + [s for s, _ in good]
    H, W = good[0][1].shape[:2]
    frames, status = module.decode_files(items, gpu_device, chunk=2, **kw)
    assert tuple(frames.shape) == (5, H, W, 3)
    got = frames.cpu().numpy()
    assert status.cpu().tolist() == [module.ST_REFUSED] * 3 + [0, 0] and not got[:3].any()
    assert np.array_equal(got[3], good[0][1]) and np.array_equal(got[4], good[1][1])
    # into the middle of a pre-filled tensor: the frames in front of the first size are zeroed, nothing outside is written
    guard = torch.full((7, H, W, 3), 0x5A, dtype=torch.uint8, device=gpu_device)
    frames, status = module.decode_files(items, gpu_device, chunk=2, out=guard[1:6], **kw)
    torch.cuda.synchronize()
    assert frames.data_ptr() == guard[1:6].data_ptr()
    assert status.cpu().tolist() == [module.ST_REFUSED] * 3 + [0, 0] and np.array_equal(frames.cpu().numpy(), got)
    assert bool((guard[0] == 0x5A).all()) and bool((guard[6] == 0x5A).all())


@pytest.mark.parametrize("module, kw", FORMATS)
def test_a_call_that_accepts_nothing(gpu_device, module, kw):
    with pytest.raises(_lib.PoseRiskHipError, match="no frame was accepted; frame 0:"):
        module.decode_files(GARBAGE[:2], gpu_device, **kw)
    with pytest.raises(_lib.PoseRiskHipError, match="no frame was accepted; frame 0:"):
        module.decode_files(GARBAGE[:2], gpu_device, chunk=1, **kw)
    frames, status = module.decode_files([], gpu_device, **kw)
    assert tuple(frames.shape) == (0, 0, 0, 3) and frames.dtype == torch.uint8 and frames.device == gpu_device
    assert tuple(status.shape) == (0,) and status.dtype == torch.int32 and status.device == gpu_device
    if module is jpeg:
        frames, status, stats = module.decode_files([], gpu_device, stats=True, **kw)
        assert tuple(frames.shape) == (0, 0, 0, 3) and tuple(status.shape) == (0,)
        assert tuple(stats.shape) == (0, 4) and stats.dtype == torch.int32 and stats.device == gpu_device


@functools.lru_cache(maxsize=None)
def _retry_jpegs(W):
    """Three W x 64 4:4:4 frames with restart intervals 0, 1, 0 -> [(file, pixels by the reference decoder)].  The middle one
    has W / 8 * 8 restart segments: more than the 64 + 2 * 1 a chunk of one frame starts with."""
    y, x = np.mgrid[0:64, 0:W]
    out = []
    for k, ri in enumerate((0, 1, 0)):
        noise = np.random.default_rng(40 + k).integers(0, 24, (64, W, 3))
        img = (np.stack([x * 3 + k * 20, y * 4, (x + y) * 2], -1) + noise).clip(0, 255).astype(np.uint8)
        s = er.encode(img, 90, "4:4:4", ri)
        out.append((s, jr.decode(s)))
    assert [len(jr.parse(s)["segments"]) for s, _ in out] == [1, W, 1] and W > 66
    return out


def _buffer_bytes(stream, segments, progressive):
    """The one buffer of a chunk that holds this file alone, with room for `segments` restart segments (one table set, and with
    `progressive` the ten scans a frame starts with)."""
    sizes = [jpeg.FRAME_DTYPE.itemsize, jpeg.SEGMENT_DTYPE.itemsize, 4, jpeg.SCAN_DTYPE.itemsize, jpeg.HUFF_DTYPE.itemsize]
    rooms = [1, segments, segments if progressive else 0, 10 if progressive else 0, 1]
    return _media.layout(len(stream), list(zip(sizes, rooms)))[1]


@pytest.mark.parametrize("entropy", jpeg.ENTROPY)
@pytest.mark.parametrize("kw", [{}, {"progressive": True}], ids=["jpeg", "jpeg-progressive"])
@pytest.mark.parametrize("W", [72, 80])
def test_jpeg_segments_outgrow_the_guess_in_a_later_chunk(gpu_device, W, kw, entropy):
    """chunk=1: chunk 1 parses twice, while chunk 0's upload may still be on its way.  chunk=3: the first chunk parses twice.
    At 72 wide the 72 segments end below the same multiple of 256 as the 66 guessed (1728 and 1584 bytes, under 1792), so the
    second parse fits the buffer of the first: whatever the file's size, that input cannot make the buffer grow.  At 80 wide
    (1920 bytes) it does, beyond what chunk 0 left and beyond chunk 1's first layout, and the file's bytes move with it."""
    cases = _retry_jpegs(W)
    if W == 80:
        progressive = bool(kw.get("progressive"))
        left, first, again = (_buffer_bytes(cases[0][0], 66, progressive), _buffer_bytes(cases[1][0], 66, progressive),
                              _buffer_bytes(cases[1][0], W, progressive))
        assert again > first and again > left, (left, first, again)
    want = np.stack([px for _, px in cases])
    for chunk in (1, 3):
        frames, status, stats = jpeg.decode_files([s for s, _ in cases], gpu_device, chunk=chunk, entropy=entropy, stats=True, **kw)
        assert status.cpu().tolist() == [0, 0, 0]
        got = frames.cpu().numpy()
        assert got.shape == (3, 64, W, 3) and np.array_equal(got, want), f"chunk={chunk}"
        assert tuple(stats.shape) == (3, 4) and stats.dtype == torch.int32
        n_subseq = stats.cpu().numpy()
        # a chunk decoded one lane per restart segment leaves its rows zero; the sub-sequence decoder counts at least one per frame
        if entropy == "serial":
            assert not n_subseq.any()
        elif entropy == "sync" or chunk == 3:                                # auto: frames 0 and 2 have no restart interval
            assert (n_subseq[:, 0] >= 1).all() and not n_subseq[:, 3].any()
        else:                                                                # auto, a frame a chunk: the middle one goes serial
            assert not n_subseq[1].any() and (n_subseq[[0, 2], 0] >= 1).all()
        plain = jpeg.decode_files([s for s, _ in cases], gpu_device, chunk=chunk, entropy=entropy, **kw)
        assert len(plain) == 2 and torch.equal(plain[0], frames) and torch.equal(plain[1], status)


def test_png_idat_ranges_outgrow_the_guess_in_a_later_chunk(gpu_device):
    W, H = 16, 8
    items, want = [], []
    for k, idat in enumerate((None, 1, None)):
        px, _ = pc.pixels_for(W, H, 2, 50 + k, "noise")
        z = pc.deflate(pc.filter_rows(px, 3, pc.ADAPTIVE))
        if idat == 1:
            assert len(z) > 18                                               # one IDAT chunk a byte: more than 16 + 2 * 1 ranges
        items.append(pc.png(W, H, 2, z, idat=idat))
        want.append(pc.expected_rgb(px, W, H, 2, None))
    for chunk in (1, 3):
        frames, status = png.decode_files(items, gpu_device, chunk=chunk)
        assert status.cpu().tolist() == [0, 0, 0]
        assert np.array_equal(frames.cpu().numpy(), np.stack(want)), f"chunk={chunk}"


@pytest.mark.parametrize("module, kw", FORMATS)
def test_out_is_checked_before_anything_is_written(gpu_device, module, kw):
    good, _ = _same_size(module)
    items = [s for s, _ in good[:3]]
    H, W = good[0][1].shape[:2]
    wrong = {"shape": torch.full((4, H, W, 3), 0x5A, dtype=torch.uint8, device=gpu_device),
             "dtype": torch.full((3, H, W, 3), 0x5A, dtype=torch.int8, device=gpu_device),
             "strides": torch.full((3, H, W, 4), 0x5A, dtype=torch.uint8, device=gpu_device)[..., :3]}
    assert tuple(wrong["strides"].shape) == (3, H, W, 3) and not wrong["strides"].is_contiguous()
    for what, out in wrong.items():
        before = out.clone()
        with pytest.raises(ValueError) as e:
            module.decode_files(items, gpu_device, out=out, **kw)
        assert str(e.value).startswith("out must be a contiguous uint8"), (what, str(e.value))
        torch.cuda.synchronize()
        assert torch.equal(out, before), f"wrong {what}: out was written"


def test_png_max_bytes_cuts_the_chunks_and_changes_nothing(gpu_device):
    cases = pc.by_size()[(160, 90)][:7]
    items = [s for _, s, _ in cases]
    sizes = [len(s) for s in items]
    W, H = 160, 90
    per_frame = (H * (1 + 4 * W) + 32) + H * W * 3                           # decode_files' estimate: workspace and output a frame
    max_bytes = 2 * per_frame + 2 * max(sizes) + 32                          # any two files fit ...
    cuts, lo = [], 0
    while lo < 7:                                                            # ... and by the rule as decode_files states it, no three
        n, total = 0, 0
        while lo + n < 7 and n < 1024 and (n == 0 or (n + 1) * per_frame + total + sizes[lo + n] + 32 <= max_bytes):
            total += sizes[lo + n]
            n += 1
        cuts.append(n)
        lo += n
    assert cuts == [2, 2, 2, 1]
    want = png.decode_files(items, gpu_device)
    got = png.decode_files(items, gpu_device, chunk=1024, max_bytes=max_bytes)
    assert want[1].cpu().tolist() == [0] * 7 and np.array_equal(want[0].cpu().numpy(), np.stack([px for _, _, px in cases]))
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
