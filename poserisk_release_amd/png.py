"""PNG frames decoded on the GPU, exact with zlib and libpng (what cv2.imread and Pillow's .convert("RGB") give): the front of
the accelerated path for a folder of lossless frames as `ffmpeg -i clip.mp4 %09d.png`, screen recorders, annotation tools and
this package's own report path write them.  The contract is in include/poserisk_hip.h (section j4); the chunk walk is
csrc/png_host.cc (host, no device), everything else csrc/png.hip over csrc/png_device.h.

The other direction -- `encode_frames`, u8 frames on the device to PNG files, section j5 -- is at the end of this file.

`list_frames` orders a folder, `parse` is the host half, `decode_files` the whole thing: file bytes and descriptors of a chunk
go through ONE pinned buffer and ONE upload (_media.decode_chunks), then pr_png_decode (gather, inflate, unfilter + Adler-32 +
colour)."""
import ctypes as C
import os

import numpy as np
import torch

from . import _lib, _media
from ._media import download_files   # noqa: F401  (buffer, nbytes) -> [bytes]: one shape of result for both encoders

# pr_png_frame, pr_png_idat as numpy records (tests compare them with the C structs); a palette is 256 x 3 bytes
FRAME_DTYPE = np.dtype([("width", "<i4"), ("height", "<i4"), ("color_type", "<i4"), ("bpp", "<i4"), ("first_idat", "<i4"),
                        ("n_idat", "<i4"), ("palette", "<i4"), ("reserved", "<i4"), ("zlib_bytes", "<i8")])
IDAT_DTYPE = np.dtype([("begin", "<i8"), ("end", "<i8")])
PALETTE_BYTES = 768
ST_REFUSED, ST_TRUNCATED, ST_BAD_CODE, ST_SIZE, ST_FILTER, ST_CHECKSUM = 1, 2, 4, 8, 16, 32
_ST_NAMES = ((ST_REFUSED, "refused (the file, its descriptor or its IDAT ranges are invalid)"),
             (ST_TRUNCATED, "the deflate stream ends early"), (ST_BAD_CODE, "the deflate stream breaks a rule of RFC 1951"),
             (ST_SIZE, "the stream does not inflate to the image's size"), (ST_FILTER, "a scanline's filter byte is above 4"),
             (ST_CHECKSUM, "the Adler-32 of the inflated bytes does not match"))
# Frames per decode call.  A frame is one serial chain of symbols on one wavefront, so the rate comes from the frames in flight
# (800 x 450, Pillow's default level: 170 / 515 / 1 058 frames/s at 64 / 256 / 1024 a call, profiles/png_decode.json); 256 keeps
# the workspace, 2.1 MB a frame at that size, at half a gigabyte.  Pass chunk=1024 where the memory is there.
DEFAULT_CHUNK = 256
DEFAULT_MAX_BYTES = 4 << 30
_EXT = (".png",)


def status_text(st):
    """The words for a pr_png_decode status."""
    return "; ".join(t for bit, t in _ST_NAMES if st & bit) or "ok"


def refusal_name(code):
    """The words for a pr_png_parse refusal."""
    return _lib.load().pr_png_refusal_name(int(code)).decode()


def list_frames(directory):
    """The frame files of `directory`: names ending in .png (any case), sorted -- position in that order is the frame index, as
    in sorted(os.listdir).  Other files (tracking.pkl, fps.txt) are ignored; a folder that also holds .jpg / .jpeg frames is
    for the caller to refuse (dropin/core/front_end.py does)."""
    return [n for n in sorted(os.listdir(directory)) if n.lower().endswith(_EXT)]


def _parse_into(data, offsets, H, W, frames, idat, palettes, pstatus):
    """pr_png_parse into caller-owned numpy arrays -> (status code, counts int32[4] = ranges, palettes, H, W)."""
    counts = np.zeros(4, np.int32)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = _lib.load().pr_png_parse(ptr(data), ptr(offsets), len(offsets) - 1, int(H), int(W), ptr(frames), ptr(idat), len(idat),
                                  ptr(palettes), len(palettes) // PALETTE_BYTES, ptr(pstatus), ptr(counts))
    return rc, counts


def parse(blobs, H=0, W=0):
    """Host half on a list of bytes objects: (frames FRAME_DTYPE[F], idat IDAT_DTYPE[N], palettes u8[P, 256, 3], parse_status
    int32[F], H, W, offsets int64[F+1]).  Refused frames have parse_status != 0 (refusal_name gives the words)."""
    offsets, data = _media.pack(blobs)
    F = len(blobs)
    frames, pstatus = np.zeros(F, FRAME_DTYPE), np.zeros(F, np.int32)
    idat_cap, pal_cap = 16 + 2 * F, 1
    while True:
        idat, palettes = np.zeros(idat_cap, IDAT_DTYPE), np.zeros(pal_cap * PALETTE_BYTES, np.uint8)
        rc, counts = _parse_into(data, offsets, H, W, frames, idat, palettes, pstatus)
        if rc != -4:                                             # PR_ERR_CAPACITY: counts says what is needed
            _lib.check(rc, "pr_png_parse")
            return (frames, idat[:counts[0]], palettes[:counts[1] * PALETTE_BYTES].reshape(-1, 256, 3), pstatus, int(counts[2]),
                    int(counts[3]), offsets)
        idat_cap, pal_cap = max(idat_cap, int(counts[0])), max(pal_cap, int(counts[1]))


def workspace_bytes(F, H, W, data_bytes):
    """Device memory a pr_png_decode call needs (0 for sizes it refuses)."""
    return int(_lib.load().pr_png_workspace_bytes(int(F), int(H), int(W), int(data_bytes)))


def _peek_size(items):
    """(H, W) of the first item that starts like a PNG (its IHDR's numbers, unchecked: only chunks are sized by them)."""
    for p in items:
        if isinstance(p, (str, os.PathLike)):
            with open(p, "rb") as f:
                head = f.read(24)
        else:
            head = bytes(p[:24])
        if len(head) == 24 and head[:8] == b"\x89PNG\r\n\x1a\n" and head[12:16] == b"IHDR":
            w, h = int.from_bytes(head[16:20], "big"), int.from_bytes(head[20:24], "big")
            if 1 <= w <= 4096 and 1 <= h <= 4096:
                return h, w
    return 0, 0


def cut_chunk(sizes, lo, chunk, per_frame, max_bytes):
    """How many of the files of `sizes` (bytes each) from `lo` on form the next chunk: at most `chunk`, and only as many as keep
    the chunk's workspace and output (`per_frame` bytes a frame, the files' bytes, 32) within `max_bytes`; at least one."""
    n, total = 0, 0
    while lo + n < len(sizes) and n < chunk and (n == 0 or (n + 1) * per_frame + total + sizes[lo + n] + 32 <= max_bytes):
        total += sizes[lo + n]
        n += 1
    return n


def decode_files(paths_or_bytes, device, bgr=False, chunk=DEFAULT_CHUNK, out=None, max_bytes=DEFAULT_MAX_BYTES):
    """Decode F PNG files (paths, or bytes objects) of one size to u8[F,H,W,3] on `device` (RGB, or BGR as cv2.imread gives with
    bgr=True; gray replicated, alpha dropped).  Returns (frames, status int32[F] on the device): status[f] != 0 marks a frame
    that was refused (bit 0; its pixels are zero) or whose stream was damaged; `bad_frames` puts the reasons into words.  The
    files are taken in chunks of at most `chunk`, cut shorter so that a chunk's workspace and its slice of the output stay
    within `max_bytes` of device memory (at least one frame a chunk).  Per chunk the bytes are read into ONE pinned host
    buffer, the parser writes its descriptors behind them in the same buffer, and ONE asynchronous copy uploads it; the decode
    neither allocates nor synchronises (include/poserisk_hip.h, pr_png_decode).  The host waits for chunk k's upload (not its
    decode) before it reads chunk k + 1 into the buffer."""
    device = _media.cuda_device(device, "decode_files", "the decoder runs")
    items = list(paths_or_bytes)
    chunk = max(int(chunk), 1)
    lib = _lib.load()
    sizes = [_media.size(p) for p in items]
    h0, w0 = _peek_size(items)
    per_frame = (h0 * (1 + 4 * w0) + 16 + 16) + h0 * w0 * 3      # workspace without the files' bytes, and the output
    idat_per_frame = 2                                           # what a frame needed so far: only ever grows

    def rooms(n):   # [frames | palettes | IDAT ranges]
        return [n, n, 16 + idat_per_frame * n]

    def regrow(n, room, counts):   # more IDAT chunks than guessed
        nonlocal idat_per_frame
        idat_per_frame = max(idat_per_frame, -(-int(counts[0]) // n))
        return [n, n, int(counts[0])]

    def sized(H, W):
        nonlocal per_frame
        per_frame = (H * (1 + 4 * W) + 32) + H * W * 3

    def decode(c):
        o_fr, o_pal, o_idat = (c.base + o for o in c.at)
        args = _lib.PngArgs(c.base, o_fr, o_idat, o_pal, c.out, c.status, c.total, c.n, c.H, c.W, int(c.counts[0]), int(c.counts[1]),
                            int(bool(bgr)))
        return workspace_bytes(c.n, c.H, c.W, c.total), lambda *ws: _lib.check(lib.pr_png_decode(args, *ws), "pr_png_decode")

    return _media.decode_chunks(
        items, device, out, cut=lambda lo: sizes[lo:lo + cut_chunk(sizes, lo, chunk, per_frame, max_bytes)],
        itemsizes=[FRAME_DTYPE.itemsize, PALETTE_BYTES, IDAT_DTYPE.itemsize], rooms=rooms, regrow=regrow,
        parse=lambda data, offsets, H, W, v, pst: _parse_into(data, offsets, H, W, v[0].view(FRAME_DTYPE), v[2].view(IDAT_DTYPE), v[1], pst),
        parser="pr_png_parse", used=0, sized=sized, decode=decode, refusal_name=refusal_name, refused=ST_REFUSED)


def bad_frames(paths_or_bytes, status):
    """[(frame index, reason)] for every frame of a decode_files call whose status is non-zero (one device -> host copy; a
    refused frame's file is parsed again on its own to name the parser's reason)."""
    return _media.bad_frames(paths_or_bytes, status, status_text, parse, refusal_name, ST_REFUSED)


# ---- the encoder (include/poserisk_hip.h, section j5): host half csrc/png_enc_host.cc, device half csrc/png_enc.hip ------------
ENC_PLAN_DTYPE = np.dtype([("width", "<i4"), ("height", "<i4"), ("filter", "<i4"), ("mode", "<i4"), ("n_segments", "<i4"),
                           ("reserved", "<i4"), ("raw_bytes", "<i8"), ("crc_pow", "<u4", (32,)), ("idat_crc_head", "<u4"),
                           ("reserved2", "<u4"), ("head", "u1", (48,)), ("tail", "u1", (16,))])   # pr_png_enc_plan
ENC_ST_OVERFLOW = 1
ENC_SEGMENT = 16384
FILTERS = {"none": 0, "sub": 1, "up": 2, "average": 3, "paeth": 4, "adaptive": 5}
MODES = {"stored": 0, "rle": 1}


def _filter_mode(filter, mode):
    f = FILTERS.get(filter, filter) if isinstance(filter, str) else filter
    m = MODES.get(mode, mode) if isinstance(mode, str) else mode
    if not isinstance(f, int) or isinstance(f, bool) or f not in FILTERS.values():
        raise ValueError(f"filter {filter!r}: one of {sorted(FILTERS)} or 0..5")
    if not isinstance(m, int) or isinstance(m, bool) or m not in MODES.values():
        raise ValueError(f"mode {mode!r}: one of {sorted(MODES)} or 0, 1")
    return int(f), int(m)


def encode_plan(filter, mode, H, W):
    """The encoder's host half: the pr_png_enc_plan of these parameters as an ENC_PLAN_DTYPE record (the file's fixed bytes,
    the CRC power table)."""
    f, m = _filter_mode(filter, mode)
    plan = np.zeros(1, ENC_PLAN_DTYPE)
    _lib.check(_lib.load().pr_png_encode_plan(f, m, int(H), int(W), plan.ctypes.data_as(C.c_void_p)), "pr_png_encode_plan")
    return plan[0]


def encode_bound(H, W):
    """A size in bytes that no PNG file of an H x W frame exceeds (a stored-mode file has exactly this size)."""
    return int(_lib.load().pr_png_encode_bound(int(H), int(W)))


def encode_workspace_bytes(F, H, W):
    """The size of the `workspace` an encode_frames call of F frames of H x W needs."""
    return int(_lib.load().pr_png_encode_workspace_bytes(int(F), int(H), int(W)))


def encode_frames(frames, filter="adaptive", mode="rle", bgr=False, capacity=None, out=None, workspace=None):
    """Encode u8[F,H,W,3] frames on the GPU (RGB, or BGR with bgr=True) to F PNG files (colour type 2, depth 8): returns (buffer
    u8[F,cap], nbytes int32[F], status int32[F]), all on the device; file f is buffer[f, :nbytes[f]].  `filter` is a name of
    FILTERS or 0..5, `mode` "rle" (distance-1 matches and dynamic codes per 16 KiB segment) or "stored".  `capacity` is the slot
    size per frame; None takes encode_bound(H, W), which no file exceeds.  A frame that does not fit a smaller slot has nbytes 0
    and status ENC_ST_OVERFLOW and its slot is untouched: encode it again with capacity=encode_bound(H, W).  `out` = (buffer,
    nbytes, status) to write into caller-owned tensors; `workspace` = a u8 device tensor of at least encode_workspace_bytes(F,
    H, W) to reuse across calls on one stream (None allocates one per call).  Asynchronous on the current stream.  The first
    call of a parameter set on a device uploads its plan and waits for that copy; every later call synchronises nothing, and
    with `out` and `workspace` given allocates nothing either, so it can be captured into a graph."""
    if not (isinstance(frames, torch.Tensor) and frames.is_cuda):
        raise _lib.PoseRiskHipError("encode_frames: the encoder runs on the GPU only (no CPU fallback)")
    if frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[-1] != 3 or not frames.is_contiguous():
        raise ValueError(f"encode_frames: frames must be a contiguous uint8 [F, H, W, 3] tensor, got {frames.dtype} {tuple(frames.shape)}")
    f, m = _filter_mode(filter, mode)
    device, (F, H, W, _) = frames.device, frames.shape
    lib = _lib.load()
    with torch.cuda.device(device):
        plan, _ = _media.device_plan(("png.encode", f, m, H, W), device, lambda: (encode_plan(f, m, H, W).tobytes(), None))
        capacity = encode_bound(H, W) if capacity is None else int(capacity)
        if out is None:
            out = (torch.empty((F, capacity), dtype=torch.uint8, device=device), torch.empty(F, dtype=torch.int32, device=device),
                   torch.empty(F, dtype=torch.int32, device=device))
        buf, nbytes, status = out
        for t, shape, dtype in ((buf, (F, capacity), torch.uint8), (nbytes, (F,), torch.int32), (status, (F,), torch.int32)):
            if tuple(t.shape) != shape or t.dtype != dtype or not t.is_contiguous() or t.device != device:
                raise ValueError(f"encode_frames: out must hold contiguous tensors {[F, capacity]} uint8, {[F]} int32, {[F]} int32 on {device}")
        if F == 0:
            return buf, nbytes, status
        need = encode_workspace_bytes(F, H, W)
        if need == 0:
            raise _lib.PoseRiskHipError(f"encode_frames: {F} frames of {W}x{H} are outside what the encoder accepts (sizes 1..4096, "
                                        "at most 65535 frames a call)")
        ws = workspace
        if ws is None:
            ws = torch.empty(need, dtype=torch.uint8, device=device)
        elif ws.dtype != torch.uint8 or ws.device != device or not ws.is_contiguous() or ws.numel() < need or ws.data_ptr() & 15:
            raise ValueError(f"encode_frames: workspace must be a contiguous, 16-byte aligned uint8 tensor of at least {need} bytes on {device}")
        stream = torch.cuda.current_stream(device)
        args = _lib.PngEncArgs(frames.data_ptr(), plan.data_ptr(), buf.data_ptr(), nbytes.data_ptr(), status.data_ptr(), capacity,
                               F, H, W, f, m, int(bool(bgr)))
        _lib.check(lib.pr_png_encode(args, ws.data_ptr(), ws.numel(), stream.cuda_stream), "pr_png_encode")
        ws.record_stream(stream)
    return buf, nbytes, status
