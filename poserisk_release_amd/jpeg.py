"""Baseline JPEG frames decoded on the GPU, bit-exact with libjpeg's default path (what cv2.imread and Pillow run): the front
of the accelerated path for a folder of frames as the reference's front end writes it (`<output>/tmp/%09d.jpg`,
lib/core/base.py:47-56, read back by CropDataset with cv2.imread).  The contract is in include/poserisk_hip.h (section j1);
the marker parser is csrc/jpeg_host.cc (host, no device), everything else csrc/jpeg.hip.

`list_frames` orders a folder, `parse` is the host half, `decode_files` the whole thing: file bytes and descriptors of a chunk
go through ONE pinned buffer and ONE upload (_media.decode_chunks), then pr_jpeg_decode.  Progressive files and files whose
components come in several scans (section j1b; csrc/jpeg_scans_host.cc, csrc/jpeg_scans.hip) are opt-in: `parse_scans` is their
host half, `decode_files(progressive=True)` sends a chunk that holds one to pr_jpeg_decode_scans.

The inverse direction (section j2; csrc/jpeg_enc.hip): `encode_frames` turns u8 frames on the device into complete baseline
JPEG files in per-frame slots, byte for byte what libjpeg writes with the standard tables; `download_files` brings only the
used bytes to the host."""
import ctypes as C
import os

import numpy as np
import torch

from . import _lib, _media
from ._media import download_files   # noqa: F401  (buffer, nbytes) -> [bytes]: one shape of result for both encoders

# pr_jpeg_frame, pr_jpeg_segment, pr_jpeg_hufftab / pr_jpeg_huff as numpy records (tests compare them with the C structs)
FRAME_DTYPE = np.dtype([("width", "<i4"), ("height", "<i4"), ("ncomp", "<i4"), ("hs", "<i4"), ("vs", "<i4"),
                        ("restart_interval", "<i4"), ("first_segment", "<i4"), ("n_segments", "<i4"), ("huff_set", "<i4"),
                        ("dc_sel", "<i4", (3,)), ("ac_sel", "<i4", (3,)), ("quant", "<u2", (3, 64))])
SEGMENT_DTYPE = np.dtype([("begin", "<i8"), ("end", "<i8"), ("frame", "<i4"), ("first_mcu", "<i4")])
HUFFTAB_DTYPE = np.dtype([("look", "<u2", (512,)), ("maxcode", "<i4", (17,)), ("valoff", "<i4", (17,)), ("vals", "u1", (256,)),
                          ("defined", "<i4")])
HUFF_DTYPE = np.dtype([("tab", HUFFTAB_DTYPE, (4,))])
# pr_jpeg_scan (section j1b: progressive and multi-scan files)
SCAN_DTYPE = np.dtype([("frame", "<i4"), ("ncomp", "<i4"), ("comp", "<i4", (3,)), ("dc_sel", "<i4", (3,)), ("ac_sel", "<i4", (3,)),
                       ("ss", "<i4"), ("se", "<i4"), ("ah", "<i4"), ("al", "<i4"), ("huff_set", "<i4"), ("restart_interval", "<i4"),
                       ("first_segment", "<i4"), ("n_segments", "<i4"), ("n_mcus", "<i4"), ("level", "<i4")])
ST_REFUSED, ST_TRUNCATED, ST_BAD_RUN, ST_BAD_CODE, ST_IDCT_RANGE, ST_COEF_RANGE = 1, 2, 4, 8, 16, 32
_ST_NAMES = ((ST_REFUSED, "refused (descriptor or segment range invalid)"), (ST_TRUNCATED, "entropy-coded data ends early"),
             (ST_BAD_RUN, "a zero run leaves the block"), (ST_BAD_CODE, "a Huffman code no table holds"),
             (ST_IDCT_RANGE, "coefficients outside the 32-bit IDCT bound"), (ST_COEF_RANGE, "a DC value outside int16"))
# Frames per decode call.  1024 was chosen for pr_jpeg_decode, for which a frame without restart markers -- what cv2.imwrite
# writes -- is one serial chain on one lane, 112 ms whether 64 or 256 of them are in flight, so that the rate was the chunk
# (571 / 2220 / 5142 frames/s at 64 / 256 / 1024; Pillow on 16 threads: 2033).  entropy="auto" now decodes such frames with
# pr_jpeg_decode_sync: decode_files gives 13.2 k / 25.2 k / 19.1 k frames/s at 64 / 256 / 1024 (profiles/jpeg_decode.json,
# DESIGN.md section 3.9), so the large chunk is no longer needed and 256 would be faster; the default is left where it was in
# this change.  Workspace 3.3 MB a frame.
DEFAULT_CHUNK = 1024
_EXT = (".jpg", ".jpeg")
# pr_jpeg_enc_plan as a numpy record
ENC_PLAN_DTYPE = np.dtype([("width", "<i4"), ("height", "<i4"), ("hs", "<i4"), ("vs", "<i4"), ("restart_interval", "<i4"),
                           ("quality", "<i4"), ("header_bytes", "<i4"), ("reserved", "<i4"), ("quant", "<u2", (2, 64)),
                           ("recip", "<u4", (2, 64)), ("dc_code", "<u2", (2, 16)), ("ac_code", "<u2", (2, 256)),
                           ("dc_len", "u1", (2, 16)), ("ac_len", "u1", (2, 256)), ("header", "u1", (640,))])
ENC_ST_OVERFLOW = 1
SUBSAMPLING = {"4:4:4": (1, 1), "4:2:2": (2, 1), "4:2:0": (2, 2)}


def status_text(st):
    """The words for a pr_jpeg_decode status."""
    return "; ".join(t for bit, t in _ST_NAMES if st & bit) or "ok"


def refusal_name(code):
    return _lib.load().pr_jpeg_refusal_name(int(code)).decode()


def scan_refusal_name(code):
    """The words for a pr_jpeg_parse_scans refusal (pr_jpeg_parse's codes and the progression rules')."""
    return _lib.load().pr_jpeg_scan_refusal_name(int(code)).decode()


def list_frames(directory):
    """The frame files of `directory`: names ending in .jpg / .jpeg (any case), sorted -- position in that order is the frame
    index, as in the reference's sorted(os.listdir) (multi_person_tracker's ImageFolder, CropDataset).  A .png among them is
    refused by name: this module decodes no PNG (a folder of PNG frames alone is png.py's).  Other files (tracking.pkl,
    fps.txt) are ignored."""
    names = sorted(os.listdir(directory))
    png = [n for n in names if n.lower().endswith(".png")]
    if png:
        raise ValueError(f"{os.path.join(directory, png[0])!r}: PNG frames are not supported (there is no PNG decoder here); "
                         "convert the frames to baseline JPEG or pass frames.npy")
    return [n for n in names if n.lower().endswith(_EXT)]


def _parse_into(data, offsets, H, W, frames, segs, huff, pstatus):
    """pr_jpeg_parse into caller-owned numpy arrays -> (status code, counts int32[4] = segments, table sets, H, W)."""
    counts = np.zeros(4, np.int32)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = _lib.load().pr_jpeg_parse(ptr(data), ptr(offsets), len(offsets) - 1, int(H), int(W), ptr(frames), ptr(segs), len(segs),
                                   ptr(huff), len(huff), ptr(pstatus), ptr(counts))
    return rc, counts


def parse(blobs, H=0, W=0):
    """Host half on a list of bytes objects: (frames FRAME_DTYPE[F], segments SEGMENT_DTYPE[S], huff HUFF_DTYPE[T],
    parse_status int32[F], H, W, offsets int64[F+1]).  Refused frames have parse_status != 0 (refusal_name gives the words)."""
    offsets, data = _media.pack(blobs)
    F = len(blobs)
    frames, pstatus = np.zeros(F, FRAME_DTYPE), np.zeros(F, np.int32)
    seg_cap, huff_cap = 64 + 2 * F, 4
    while True:
        segs, huff = np.zeros(seg_cap, SEGMENT_DTYPE), np.zeros(huff_cap, HUFF_DTYPE)
        rc, counts = _parse_into(data, offsets, H, W, frames, segs, huff, pstatus)
        if rc != -4:                                             # PR_ERR_CAPACITY: counts says what is needed
            _lib.check(rc, "pr_jpeg_parse")
            return frames, segs[:counts[0]], huff[:counts[1]], pstatus, int(counts[2]), int(counts[3]), offsets
        seg_cap, huff_cap = max(seg_cap, int(counts[0])), max(huff_cap, int(counts[1]))


def _parse_scans_into(data, offsets, H, W, frames, segs, seg_scan, huff, scans, pstatus):
    """pr_jpeg_parse_scans into caller-owned numpy arrays -> (status code, counts int32[8] = segments, table sets, H, W, scans,
    levels, frames with more than one scan, 0)."""
    counts = np.zeros(8, np.int32)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = _lib.load().pr_jpeg_parse_scans(ptr(data), ptr(offsets), len(offsets) - 1, int(H), int(W), ptr(frames), ptr(segs),
                                         ptr(seg_scan), len(segs), ptr(huff), len(huff), ptr(scans), len(scans), ptr(pstatus),
                                         ptr(counts))
    return rc, counts


def parse_scans(blobs, H=0, W=0):
    """The scan-aware host half (pr_jpeg_parse_scans: progressive files and sequential files in several scans beside
    everything `parse` accepts) on a list of bytes objects: `parse`'s tuple (frames, segments, huff, parse_status, H, W,
    offsets) followed by scans SCAN_DTYPE[N], segment_scan int32[S] (segment i belongs to scans[segment_scan[i]]), the number
    of levels and the number of frames with more than one scan.  scan_refusal_name gives a refusal's words."""
    offsets, data = _media.pack(blobs)
    F = len(blobs)
    frames, pstatus = np.zeros(F, FRAME_DTYPE), np.zeros(F, np.int32)
    seg_cap, huff_cap, scan_cap = 64 + 16 * F, 4 + F, 16 * F
    while True:
        segs, seg_scan = np.zeros(seg_cap, SEGMENT_DTYPE), np.zeros(seg_cap, np.int32)
        huff, scans = np.zeros(huff_cap, HUFF_DTYPE), np.zeros(scan_cap, SCAN_DTYPE)
        rc, counts = _parse_scans_into(data, offsets, H, W, frames, segs, seg_scan, huff, scans, pstatus)
        if rc != -4:                                             # PR_ERR_CAPACITY: counts says what is needed
            _lib.check(rc, "pr_jpeg_parse_scans")
            return (frames, segs[:counts[0]], huff[:counts[1]], pstatus, int(counts[2]), int(counts[3]), offsets, scans[:counts[4]],
                    seg_scan[:counts[0]], int(counts[5]), int(counts[6]))
        seg_cap, huff_cap, scan_cap = max(seg_cap, int(counts[0])), max(huff_cap, int(counts[1])), max(scan_cap, int(counts[4]))


def workspace_bytes(F, H, W):
    return int(_lib.load().pr_jpeg_workspace_bytes(int(F), int(H), int(W)))


ENTROPY = ("auto", "serial", "sync")
SYNC_STATS_DTYPE = np.dtype([("n_subseq", "<i4"), ("rounds", "<i4"), ("fell_back", "<i4"), ("reserved", "<i4")])   # pr_jpeg_sync_stats


def _sync_opts(sync_opts):
    """None (the build's defaults) or (subseq_bytes, max_rounds) -> what pr_jpeg_decode_sync takes."""
    if sync_opts is None:
        return None
    S, R = sync_opts
    return _lib.JpegSyncOpts(int(S), int(R))


def sync_workspace_bytes(F, H, W, data_bytes, n_segments, sync_opts=None):
    """Device memory a pr_jpeg_decode_sync call needs (0 for sizes or options it refuses): workspace_bytes(F, H, W) plus the
    sub-sequences' states.  sync_opts: None, or (subseq_bytes, max_rounds)."""
    return int(_lib.load().pr_jpeg_sync_workspace_bytes(int(F), int(H), int(W), int(data_bytes), int(n_segments), _sync_opts(sync_opts)))


def decode_files(paths_or_bytes, device, bgr=False, chunk=DEFAULT_CHUNK, out=None, entropy="auto", stats=False, sync_opts=None,
                 progressive=False):
    """Decode F baseline JPEG files (paths, or bytes objects) of one size to u8[F,H,W,3] on `device` (RGB, or BGR as cv2.imread
    gives with bgr=True).  Returns (frames, status int32[F] on the device): status[f] != 0 marks a frame that was refused
    (bit 0; its pixels are zero) or whose stream was damaged; `bad_frames` puts the reasons into words.  Per chunk of `chunk`
    files the bytes are read into ONE pinned host buffer, the parser writes its descriptors behind them in the same buffer, and
    ONE asynchronous copy uploads it; the decode neither allocates nor synchronises (include/poserisk_hip.h, pr_jpeg_decode).
    The host waits for chunk k's upload (not its decode) before it reads chunk k + 1 into the buffer.
    `entropy`: "serial" decodes with one lane per restart segment (pr_jpeg_decode), "sync" with one lane per sub-sequence of a
    segment (pr_jpeg_decode_sync: what frames without restart markers need), "auto" picks per chunk: sync where any accepted
    frame of the chunk has no restart interval, serial otherwise.  `sync_opts` = (subseq_bytes, max_rounds) instead of the
    build's defaults.  stats=True returns (frames, status, stats): a SYNC_STATS_DTYPE int32[F, 4] tensor on the device, per
    frame (n_subseq, rounds, fell_back, 0); all zero for frames of a chunk that went the serial way.
    `progressive`: False refuses progressive files and files whose components come in several scans, as ever.  True parses
    every chunk with pr_jpeg_parse_scans (section j1b): a chunk WITHOUT such a frame takes exactly the path above (the same
    records, entries and `entropy` rule); a chunk with at least one is decoded by pr_jpeg_decode_scans, one launch per level of
    the scan scripts, its baseline frames one lane per restart segment whatever `entropy` says, its `stats` rows zero.  For
    such a call `bad_frames(..., progressive=True)` names the refusals."""
    if entropy not in ENTROPY:
        raise ValueError(f"decode_files: entropy = {entropy!r}: one of {ENTROPY}")
    device = _media.cuda_device(device, "decode_files", "the decoder runs")
    items = list(paths_or_bytes)
    F, chunk = len(items), max(int(chunk), 1)
    lib, opts = _lib.load(), _sync_opts(sync_opts)
    # what a frame needed so far: these only grow, so that later chunks start from what an earlier one needed (a folder one
    # encoder wrote has one restart interval)
    seg_per_frame, scan_per_frame, huff_room, sync_stats = 2, (10 if progressive else 0), 0, None

    def rooms(n):
        """[frames | segments | segments' scans | scans | table sets]; the two in the middle stay empty without `progressive`."""
        nonlocal huff_room
        huff_room = max(huff_room, n)
        seg_room = 64 + seg_per_frame * n
        return [n, seg_room, seg_room if progressive else 0, scan_per_frame * n, huff_room]

    def regrow(n, room, counts):   # more restart segments (scans, table sets) than guessed
        nonlocal seg_per_frame, scan_per_frame, huff_room
        seg_room, scan_room = int(counts[0]), room[3]
        seg_per_frame = max(seg_per_frame, -(-seg_room // n))
        if progressive:
            scan_room, huff_room = max(scan_room, int(counts[4])), max(huff_room, int(counts[1]))
            scan_per_frame = max(scan_per_frame, -(-scan_room // n))
        return [n, seg_room, seg_room if progressive else 0, scan_room, huff_room]

    def parse_chunk(data, offsets, H, W, views, pst):
        fr, segs, seg_scan, scans, huff = (v.view(t) for v, t in zip(views, (FRAME_DTYPE, SEGMENT_DTYPE, np.int32, SCAN_DTYPE, HUFF_DTYPE)))
        if progressive:
            return _parse_scans_into(data, offsets, H, W, fr, segs, seg_scan, huff, scans, pst)
        return _parse_into(data, offsets, H, W, fr, segs, huff, pst)

    def sized(H, W):
        nonlocal sync_stats
        sync_stats = torch.zeros((F, 4), dtype=torch.int32, device=device) if stats else None

    def decode(c):
        """serial, sync or scans for this chunk, from what the parser counted and the accepted frames' restart intervals"""
        o_fr, o_seg, o_ss, o_sc, o_huff = (c.base + o for o in c.at)
        n_segs, n_huff = int(c.counts[0]), int(c.counts[1])
        ok = c.views[0].view(FRAME_DTYPE)[c.pstatus == 0]
        multi = progressive and int(c.counts[6]) > 0
        sync = not multi and (entropy == "sync" or (entropy == "auto" and bool((ok["restart_interval"] == 0).any())))
        need = sync_workspace_bytes(c.n, c.H, c.W, c.total, n_segs, sync_opts) if sync else workspace_bytes(c.n, c.H, c.W)
        if sync and need == 0:
            raise _lib.PoseRiskHipError(f"decode_files: sync_opts = {sync_opts!r}: subseq_bytes is a multiple of 4 in 16..4096 "
                                        "(or 0 for the default), max_rounds 1..64")
        args = _lib.JpegArgs(c.base, o_fr, o_seg, o_huff, c.out, c.status, c.total, c.n, c.H, c.W, n_segs, n_huff, int(bool(bgr)))
        if multi:
            sargs = _lib.JpegScansArgs(args, o_sc, o_ss, int(c.counts[4]), int(c.counts[5]))
            return need, lambda *ws: _lib.check(lib.pr_jpeg_decode_scans(sargs, *ws), "pr_jpeg_decode_scans")
        if sync:
            st_ptr = sync_stats[c.lo:c.lo + c.n].data_ptr() if stats else None
            return need, lambda *ws: _lib.check(lib.pr_jpeg_decode_sync(args, opts, st_ptr, *ws), "pr_jpeg_decode_sync")
        return need, lambda *ws: _lib.check(lib.pr_jpeg_decode(args, *ws), "pr_jpeg_decode")

    frames_out, status = _media.decode_chunks(
        items, device, out, cut=lambda lo: [_media.size(p) for p in items[lo:lo + chunk]], rooms=rooms, regrow=regrow,
        itemsizes=[FRAME_DTYPE.itemsize, SEGMENT_DTYPE.itemsize, 4, SCAN_DTYPE.itemsize, HUFF_DTYPE.itemsize], parse=parse_chunk,
        parser="pr_jpeg_parse_scans" if progressive else "pr_jpeg_parse", used=1, sized=sized, decode=decode,
        refusal_name=scan_refusal_name, refused=ST_REFUSED)
    if not stats:
        return frames_out, status
    return frames_out, status, sync_stats if F else torch.zeros((0, 4), dtype=torch.int32, device=device)


def bad_frames(paths_or_bytes, status, progressive=False):
    """[(frame index, reason)] for every frame of a decode_files call whose status is non-zero (one device -> host copy; a
    refused frame's file is parsed again on its own to name the parser's reason: with progressive=True, as the call was made,
    by the scan-aware parser)."""
    return _media.bad_frames(paths_or_bytes, status, status_text, parse_scans if progressive else parse, scan_refusal_name, ST_REFUSED)


def encode_plan(quality, subsampling, restart_interval, H, W):
    """The encoder's host half: the pr_jpeg_enc_plan of these parameters as an ENC_PLAN_DTYPE record (tables, header bytes)."""
    if subsampling not in SUBSAMPLING:
        raise ValueError(f"subsampling {subsampling!r}: one of {sorted(SUBSAMPLING)}")
    hs, vs = SUBSAMPLING[subsampling]
    plan = np.zeros(1, ENC_PLAN_DTYPE)
    _lib.check(_lib.load().pr_jpeg_encode_plan(int(quality), hs, vs, int(restart_interval), int(H), int(W),
                                               plan.ctypes.data_as(C.c_void_p)), "pr_jpeg_encode_plan")
    return plan[0]


def encode_bound(H, W, subsampling="4:2:0", restart_interval=-1):
    """A size in bytes that no file of these parameters exceeds.  It depends on the sampling and the restart interval: pass the
    ones the encode_frames call uses (restart_rows=1 is interval -1, restart_rows=0 is 0)."""
    if subsampling not in SUBSAMPLING:
        raise ValueError(f"subsampling {subsampling!r}: one of {sorted(SUBSAMPLING)}")
    hs, vs = SUBSAMPLING[subsampling]
    return int(_lib.load().pr_jpeg_encode_bound(int(H), int(W), hs, vs, int(restart_interval)))


def encode_frames(frames, quality=90, subsampling="4:2:0", restart_rows=1, bgr=False, capacity=None, out=None, workspace=None):
    """Encode u8[F,H,W,3] frames on the GPU (RGB, or BGR with bgr=True) to F baseline JPEG files: returns (buffer u8[F,cap],
    nbytes int32[F], status int32[F]), all on the device; file f is buffer[f, :nbytes[f]], header and EOI included.
    restart_rows=1 writes a restart marker per MCU row (the streams this package's decoder is fast on), 0 none.  `capacity` is
    the slot size per frame; None takes min(encode_bound, 4096 + H * W * 3 // 2), which photographs and rendered canvases stay
    far below at any quality.  A frame that does not fit has nbytes 0 and status ENC_ST_OVERFLOW and its slot is untouched:
    encode it again with capacity=encode_bound(H, W, subsampling, -1 if restart_rows else 0).  `out` = (buffer, nbytes, status)
    to write into caller-owned tensors; `workspace` = a u8 device tensor of at least encode_workspace_bytes(...) to reuse across
    calls on one stream (None allocates one per call).  Asynchronous on the current stream.  The first call of a parameter set
    on a device uploads its plan and waits for that copy (_media.device_plan); every later call synchronises nothing, and with `out`
    and `workspace` given allocates nothing either, so it can be captured into a graph."""
    if not (isinstance(frames, torch.Tensor) and frames.is_cuda):
        raise _lib.PoseRiskHipError("encode_frames: the encoder runs on the GPU only (no CPU fallback)")
    if frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[-1] != 3 or not frames.is_contiguous():
        raise ValueError(f"encode_frames: frames must be a contiguous uint8 [F, H, W, 3] tensor, got {frames.dtype} {tuple(frames.shape)}")
    if restart_rows not in (0, 1):
        raise ValueError(f"encode_frames: restart_rows = {restart_rows!r}: 1 (a marker per MCU row) or 0 (none)")
    if subsampling not in SUBSAMPLING:
        raise ValueError(f"subsampling {subsampling!r}: one of {sorted(SUBSAMPLING)}")
    device, (F, H, W, _) = frames.device, frames.shape
    hs, vs = SUBSAMPLING[subsampling]
    ri = -1 if restart_rows else 0
    lib = _lib.load()
    with torch.cuda.device(device):
        key = (int(quality), subsampling, ri, H, W)
        plan, _ = _media.device_plan(("jpeg.encode",) + key, device, lambda: (encode_plan(*key).tobytes(), None))
        if capacity is None:
            capacity = min(encode_bound(H, W, subsampling, ri), 4096 + H * W * 3 // 2)
        capacity = int(capacity)
        if out is None:
            out = (torch.empty((F, capacity), dtype=torch.uint8, device=device), torch.empty(F, dtype=torch.int32, device=device),
                   torch.empty(F, dtype=torch.int32, device=device))
        buf, nbytes, status = out
        for t, shape, dtype in ((buf, (F, capacity), torch.uint8), (nbytes, (F,), torch.int32), (status, (F,), torch.int32)):
            if tuple(t.shape) != shape or t.dtype != dtype or not t.is_contiguous() or t.device != device:
                raise ValueError(f"encode_frames: out must hold contiguous tensors {[F, capacity]} uint8, {[F]} int32, {[F]} int32 on {device}")
        if F == 0:
            return buf, nbytes, status
        need = int(lib.pr_jpeg_encode_workspace_bytes(F, H, W, hs, vs, ri, capacity))
        if need == 0:
            raise _lib.PoseRiskHipError(f"encode_frames: {F} frames of {W}x{H} with capacity {capacity} are outside what the encoder "
                                        "accepts (sizes 16..4096, at most 65535 frames a call, capacity below 2^31)")
        ws = workspace
        if ws is None:
            ws = torch.empty(need, dtype=torch.uint8, device=device)
        elif ws.dtype != torch.uint8 or ws.device != device or not ws.is_contiguous() or ws.numel() < need or ws.data_ptr() & 15:
            raise ValueError(f"encode_frames: workspace must be a contiguous, 16-byte aligned uint8 tensor of at least {need} bytes on {device}")
        stream = torch.cuda.current_stream(device)
        args = _lib.JpegEncArgs(frames.data_ptr(), plan.data_ptr(), buf.data_ptr(), nbytes.data_ptr(), status.data_ptr(), capacity,
                                F, H, W, hs, vs, ri, int(bool(bgr)))
        _lib.check(lib.pr_jpeg_encode(args, ws.data_ptr(), ws.numel(), stream.cuda_stream), "pr_jpeg_encode")
        ws.record_stream(stream)
    return buf, nbytes, status


def encode_workspace_bytes(F, H, W, subsampling="4:2:0", restart_rows=1, capacity=None):
    """The size of the `workspace` an encode_frames call of these parameters needs (capacity None: the default slot)."""
    if subsampling not in SUBSAMPLING:
        raise ValueError(f"subsampling {subsampling!r}: one of {sorted(SUBSAMPLING)}")
    hs, vs = SUBSAMPLING[subsampling]
    ri = -1 if restart_rows else 0
    if capacity is None:
        capacity = min(encode_bound(H, W, subsampling, ri), 4096 + H * W * 3 // 2)
    return int(_lib.load().pr_jpeg_encode_workspace_bytes(int(F), int(H), int(W), hs, vs, ri, int(capacity)))
