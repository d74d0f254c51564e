"""YUV4MPEG2 (`.y4m`) video read and written on the GPU: the raw planar stream that `ffmpeg -f yuv4mpegpipe`, mpv, GStreamer's y4menc, x264
and the AV1 tools read and write, so any codec a decoder can pipe out reaches the front end without touching a disk and without
being recompressed.  The contract is in include/poserisk_hip.h (section j6); the host half (csrc/y4m_host.cc) reads the
syntax, the device half (csrc/yuv.hip) does chroma upsampling, the colour matrix and the front end's downscale in one kernel.

    is_y4m         does a file begin with the stream signature?
    parse_header   bytes -> Info (size, frame rate, chroma layout, range, header and frame bytes)
    Reader         a path, a binary file object or "-" (standard input) -> chunks of the stream in pinned host memory
    yuv_frames     a chunk on the device + payload offsets -> u8[F,h,w,3] on the device (pr_yuv_frames)
    decode         a Reader, a path or bytes -> u8[F,h,w,3] on the device
    write          planes -> a stream (for tests and users; no GPU work)
    stream_header  the stream header line
    encode_frames  u8[F,H,W,3] on the device -> the frames' stream bytes on the device (pr_yuv_encode; section j7, csrc/yuv_enc.hip)
    Writer         RGB frames on the device -> a path, a binary file object, "-" (standard output) or an encoder child process

    ffmpeg -i clip.mp4 -f yuv4mpegpipe -pix_fmt yuv420p - | python -m poserisk_release_amd.frontend prepare - frames_dir
    y4m.Writer(command=["ffmpeg", "-y", "-f", "yuv4mpegpipe", "-i", "-", "-c:v", "libx264", "out.mp4"], width=W, height=H)"""
import collections
import ctypes as C
import io
import os
import sys

import numpy as np
import torch

from . import _lib, _media
from ._child import Child

CHROMAS = ("420jpeg", "420mpeg2", "422", "444", "mono")        # index = PR_Y4M_C*
MATRICES = {"601": 0, "709": 1}                                # PR_YUV_*
MAX_FRAME_HEADER = 256                                         # PR_Y4M_MAX_FRAME_HEADER
MAX_HEADER = 1024                                              # PR_Y4M_MAX_HEADER
MAX_CHUNK = 256
SIGNATURE = b"YUV4MPEG2 "
# decode(fused=None) takes this: measured on one MI355X (profiles/y4m_frontend.json)
FUSED_DEFAULT = True

Info = collections.namedtuple("Info", "width height fps_num fps_den fps chroma full_range header_bytes frame_bytes")


def refusal_name(code):
    return _lib.load().pr_y4m_refusal_name(int(code)).decode()


def is_y4m(path):
    """True for a regular file that begins with `YUV4MPEG2 `."""
    try:
        with open(path, "rb") as f:
            return f.read(len(SIGNATURE)) == SIGNATURE
    except OSError:
        return False


def _raw_info(data):
    data = bytes(data[:MAX_HEADER])
    raw = _lib.Y4mInfo()
    rc = _lib.load().pr_y4m_parse_header(data, len(data), C.byref(raw))
    if rc > 0:
        raise ValueError(f"not a YUV4MPEG2 stream this reader takes: {refusal_name(rc)}")
    _lib.check(rc, "pr_y4m_parse_header")
    return raw


def _info(raw):
    fps = raw.fps_num / raw.fps_den if raw.fps_num and raw.fps_den else 30.0
    return Info(raw.width, raw.height, raw.fps_num, raw.fps_den, fps, CHROMAS[raw.chroma], None if raw.full_range < 0 else bool(raw.full_range),
                raw.header_bytes, raw.frame_bytes)


def parse_header(data):
    """The stream header at the start of `data` (bytes; only the first 1024 are looked at) -> Info.  fps is num / den, 30.0 for
    an absent or 0:0 field; full_range is True, False or None (no XCOLORRANGE).  A refusal raises ValueError with its name."""
    return _info(_raw_info(data))


def index(buf, info, max_frames=1 << 30):
    """`buf` (bytes or a uint8 array) begins at a FRAME header -> (payload offsets int64[m] of the complete frames, bytes
    consumed): pr_y4m_index."""
    a = np.frombuffer(buf, np.uint8) if not isinstance(buf, np.ndarray) else buf
    raw = _lib.Y4mInfo(info.width, info.height, info.fps_num, info.fps_den, CHROMAS.index(info.chroma),
                       -1 if info.full_range is None else int(info.full_range), info.header_bytes, 0, info.frame_bytes)
    cap = int(min(max_frames, a.size // (info.frame_bytes + 6) + 1))
    offsets = np.zeros(max(cap, 1), np.int64)
    n, used = C.c_int32(0), C.c_int64(0)
    rc = _lib.load().pr_y4m_index(a.ctypes.data_as(C.c_void_p), a.size, C.byref(raw), offsets.ctypes.data_as(C.c_void_p), cap,
                                  C.byref(n), C.byref(used))
    if rc > 0:
        raise ValueError(_lib.load().pr_last_error().decode("utf-8", "replace"))
    _lib.check(rc, "pr_y4m_index")
    return offsets[:n.value], int(used.value)


def yuv_plan(matrix, full_range):
    """pr_yuv_plan -> (cy, crv, cbu, cgu, cgv, yo)."""
    if matrix not in MATRICES:
        raise ValueError(f"matrix {matrix!r} is not known: '601' or '709' ('auto' is resolved by decode)")
    plan = _lib.YuvCoeffs()
    _lib.check(_lib.load().pr_yuv_plan(MATRICES[matrix], int(bool(full_range)), C.byref(plan)), "pr_yuv_plan")
    return plan.cy, plan.crv, plan.cbu, plan.cgu, plan.cgv, plan.yo


class Reader:
    """A YUV4MPEG2 stream from a path, a binary file object or "-" (standard input).  The header is read on construction
    (ValueError names a refusal): .width, .height, .fps, .chroma, .full_range (True | False | None), .info.  `frames_bound` is
    an upper bound of the frame count where the source is a regular file (its length is known), else None."""

    def __init__(self, src):
        self._own = False
        if isinstance(src, (str, os.PathLike)) and os.fspath(src) != "-":
            self.path, self._f, self._own = os.fspath(src), open(src, "rb"), True
        elif isinstance(src, (str, os.PathLike)):
            self.path, self._f = "<stdin>", sys.stdin.buffer
        else:
            self.path, self._f = getattr(src, "name", "<stream>"), src
        head = bytearray()
        while len(head) < MAX_HEADER and not head.endswith(b"\n"):          # a pipe cannot be read ahead and put back
            byte = self._f.read(1)
            if not byte:
                break
            head += byte
        try:
            self._raw = _raw_info(bytes(head))
        except ValueError as e:
            self.close()
            raise ValueError(f"{self.path!r}: {e}") from None
        self.info = _info(self._raw)
        self.width, self.height, self.fps, self.chroma, self.full_range = (self.info.width, self.info.height, self.info.fps,
                                                                           self.info.chroma, self.info.full_range)
        self.frames_read = 0
        self.frames_bound = None
        try:
            import stat
            st = os.fstat(self._f.fileno())
            if stat.S_ISREG(st.st_mode):
                self.frames_bound = max(0, (st.st_size - self._f.tell()) // (self.info.frame_bytes + 6))
        except (OSError, AttributeError, io.UnsupportedOperation):
            if isinstance(self._f, io.BytesIO):
                self.frames_bound = max(0, (len(self._f.getbuffer()) - self._f.tell()) // (self.info.frame_bytes + 6))

    def close(self):
        if self._own:
            self._f.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def chunk_bytes(self, n):
        """Host (and device) bytes of a chunk of n frames: the frames with the longest FRAME headers this reader takes."""
        return int(n) * (self.info.frame_bytes + MAX_FRAME_HEADER)

    def chunks(self, n):
        """Yields (u8 tensor in pinned host memory: the chunk's stream bytes, beginning at a FRAME header; offsets int64[m]:
        its frames' payload offsets), m <= n, until the stream ends.  Two pinned buffers are filled alternately, so reading the
        next chunk overlaps the upload of the previous one: a chunk's tensor stays valid until the chunk after the next is asked
        for (a consumer that uploads asynchronously finishes chunk k's upload before it asks for chunk k + 2).  An incomplete
        last frame raises ValueError naming its index.  Without a GPU the buffers are ordinary host memory."""
        n = max(1, int(n))
        cap = self.chunk_bytes(n)
        pin = torch.cuda.is_available()
        bufs = [torch.empty(cap, dtype=torch.uint8, pin_memory=pin) for _ in range(2)]
        views = [b.numpy() for b in bufs]
        carry, used, which, eof = 0, 0, 0, False
        while True:
            view, filled = views[which], carry
            if carry:                                 # what the previous chunk left behind its last complete frame
                view[:carry] = views[which ^ 1][used:used + carry]
            while filled < cap and not eof:
                got = self._f.readinto(memoryview(view)[filled:cap])
                if not got:
                    eof = True
                else:
                    filled += got
            try:
                offsets, used = index(view[:filled], self.info, n)
            except ValueError as e:
                raise ValueError(f"{self.path!r}: frame {self.frames_read + _frame_in_error(str(e))}: "
                                 f"{refusal_name(12)}") from None
            if len(offsets) == 0:
                if filled:
                    raise ValueError(f"{self.path!r}: frame {self.frames_read} is incomplete: the stream ends {filled} bytes into it "
                                     f"(a frame is its FRAME header and {self.info.frame_bytes} bytes)")
                return
            carry = filled - used
            self.frames_read += len(offsets)
            yield bufs[which][:used], offsets
            which ^= 1


def _frame_in_error(text):
    import re
    m = re.search(r"frame (\d+)", text)
    return int(m.group(1)) if m else 0


def _check_out(out, shape, device, what):
    if tuple(out.shape) != tuple(shape) or out.dtype != torch.uint8 or not out.is_contiguous() or out.device != device:
        raise ValueError(f"{what}: out must be a contiguous uint8 {list(shape)} tensor on {device}")


def yuv_frames(data, offsets, H, W, chroma, plan, bgr=False, size=None, out=None):
    """pr_yuv_frames: `data` u8[n] on the device (a chunk of the stream), `offsets` int64[F] on the device (payload offsets in
    it), `plan` yuv_plan's integers -> u8[F,H,W,3], or with size = (h, w) u8[F,h,w,3], downscaled by the front end's contract in
    the same kernel.  Asynchronous on the current stream; with `out` given and the size pair seen before it allocates and
    synchronises nothing."""
    from . import frontend
    if not (isinstance(data, torch.Tensor) and data.is_cuda and isinstance(offsets, torch.Tensor) and offsets.is_cuda):
        raise _lib.PoseRiskHipError("yuv_frames: the conversion runs on the GPU only (no CPU fallback)")
    if data.dtype != torch.uint8 or data.dim() != 1 or not data.is_contiguous():
        raise ValueError(f"yuv_frames: data must be a contiguous 1-D uint8 tensor, got {data.dtype} {tuple(data.shape)}")
    if offsets.dtype != torch.int64 or offsets.dim() != 1 or not offsets.is_contiguous() or offsets.device != data.device:
        raise ValueError(f"yuv_frames: offsets must be a contiguous 1-D int64 tensor on {data.device}")
    device, F = data.device, int(offsets.shape[0])
    H, W = int(H), int(W)
    h, w = (H, W) if size is None else (int(size[0]), int(size[1]))
    a = _lib.YuvArgs()
    a.plan = _lib.YuvCoeffs(*[int(v) for v in plan])
    a.F, a.H, a.W, a.chroma, a.bgr = F, H, W, CHROMAS.index(chroma), int(bool(bgr))
    with torch.cuda.device(device):
        if size is not None:
            tables, mode = frontend._resize_tables((H, W, h, w), device)
            base = tables.data_ptr()
            a.xofs, a.xcoef, a.yofs, a.ycoef = base, base + 4 * w + 4 * h, base + 4 * w, base + 8 * w + 4 * h
            a.h, a.w, a.mode = h, w, mode
        if out is None:
            out = torch.empty((F, h, w, 3), dtype=torch.uint8, device=device)
        _check_out(out, (F, h, w, 3), device, "yuv_frames")
        a.data, a.data_bytes, a.offsets, a.dst = data.data_ptr(), int(data.shape[0]), offsets.data_ptr(), out.data_ptr()
        _lib.check(_lib.load().pr_yuv_frames(C.byref(a), torch.cuda.current_stream(device).cuda_stream), "pr_yuv_frames")
    return out


def chunk_frames(info, max_bytes, unfused_rgb=False):
    """Frames per call: the largest count <= 256 whose chunk (and, for the two-step path, source-size RGB) fits max_bytes."""
    per = info.frame_bytes + MAX_FRAME_HEADER + 8 + (info.width * info.height * 3 if unfused_rgb else 0)
    return max(1, min(MAX_CHUNK, int(max_bytes) // per))


def decode(src, device, matrix="601", full_range=None, bgr=False, size=None, fused=None, max_bytes=16 << 30, chunk=None):
    """A Reader, a path, "-", a binary file object or the stream's bytes -> u8[F,h,w,3] on `device`, RGB (BGR with bgr=True).
    matrix: "601" (the default: what swscale's unconfigured conversion uses at every size), "709", or "auto" (709 above 576
    rows).  full_range None takes the header's XCOLORRANGE (limited when it says nothing).  size = (h, w): downscaled by the
    front end's contract (frontend.resize_frames' bits) -- in the conversion kernel itself with fused=True, by
    frontend.resize_frames after a conversion at the source size with fused=False; None takes FUSED_DEFAULT.  The stream is read
    chunk by chunk (`chunk` frames, else what max_bytes allows, at most 256) into pinned memory, uploaded and converted while
    the next chunk is read.  A regular file's result is sized from its length; a pipe's chunks are concatenated once."""
    from . import frontend
    device = _media.cuda_device(device, "y4m.decode", "the conversion runs")
    if isinstance(src, (bytes, bytearray, memoryview)):
        src = io.BytesIO(bytes(src))
    reader = src if isinstance(src, Reader) else Reader(src)
    info = reader.info
    H, W = info.height, info.width
    if matrix == "auto":
        matrix = "709" if H > 576 else "601"
    full = bool(info.full_range) if full_range is None else bool(full_range)
    plan = yuv_plan(matrix, full)
    fused = FUSED_DEFAULT if fused is None else bool(fused)
    h, w = (H, W) if size is None else (int(size[0]), int(size[1]))
    if h < 1 or w < 1:
        raise ValueError(f"{reader.path!r}: {W} x {H} frames would become {w} x {h}")
    scaled = (h, w) != (H, W)
    two_step = scaled and not fused
    n = int(chunk) if chunk else chunk_frames(info, max_bytes, two_step)
    if reader.frames_bound is not None:
        n = max(1, min(n, reader.frames_bound))
    with torch.cuda.device(device):
        stream = torch.cuda.current_stream(device)
        staged = torch.empty(reader.chunk_bytes(n), dtype=torch.uint8, device=device)
        staged_offsets = torch.empty(n, dtype=torch.int64, device=device)
        rgb = torch.empty((n, H, W, 3), dtype=torch.uint8, device=device) if two_step else None
        result = None if reader.frames_bound is None else torch.empty((reader.frames_bound, h, w, 3), dtype=torch.uint8, device=device)
        parts, done, uploaded = [], 0, []
        for data, offsets in reader.chunks(n):
            m = len(offsets)
            if result is not None and done + m > result.shape[0]:
                raise ValueError(f"{reader.path!r}: the stream grew while it was read")
            staged[:data.shape[0]].copy_(data, non_blocking=True)
            host_offsets = torch.from_numpy(offsets).pin_memory() if data.is_pinned() else torch.from_numpy(offsets)
            staged_offsets[:m].copy_(host_offsets, non_blocking=True)
            into = result[done:done + m] if result is not None else torch.empty((m, h, w, 3), dtype=torch.uint8, device=device)
            if two_step:
                yuv_frames(staged[:data.shape[0]], staged_offsets[:m], H, W, info.chroma, plan, bgr=bgr, out=rgb[:m])
                frontend.resize_frames(rgb[:m], h, w, out=into)
            else:
                yuv_frames(staged[:data.shape[0]], staged_offsets[:m], H, W, info.chroma, plan, bgr=bgr, size=(h, w) if scaled else None,
                           out=into)
            if result is None:
                parts.append(into)
            done += m
            event = torch.cuda.Event()
            event.record(stream)
            uploaded.append((event, host_offsets))
            if len(uploaded) > 1:                     # the chunk before this one used the buffer the next read fills
                uploaded.pop(0)[0].synchronize()
        if result is not None:
            return result[:done]
        if not parts:
            return torch.empty((0, h, w, 3), dtype=torch.uint8, device=device)
        return parts[0] if len(parts) == 1 else torch.cat(parts)


def write(dst, Y, U=None, V=None, fps=30.0, chroma="420jpeg", full_range=None, frame_fields=b""):
    """Planes -> a YUV4MPEG2 stream.  Y u8[F,H,W]; U, V u8[F,ch,cw] (None for chroma "mono"); fps a number or (num, den);
    full_range True | False writes XCOLORRANGE, None leaves it out.  `dst` is a path or a binary file object.  No GPU work."""
    Y = np.ascontiguousarray(Y, np.uint8)
    F, H, W = Y.shape
    if chroma not in CHROMAS:
        raise ValueError(f"chroma {chroma!r} is not one of {CHROMAS}")
    cw = (W + 1) // 2 if chroma in ("420jpeg", "420mpeg2", "422") else W
    ch = (H + 1) // 2 if chroma in ("420jpeg", "420mpeg2") else H
    if chroma != "mono":
        U, V = np.ascontiguousarray(U, np.uint8), np.ascontiguousarray(V, np.uint8)
        if U.shape != (F, ch, cw) or V.shape != (F, ch, cw):
            raise ValueError(f"{chroma} planes of {W} x {H} frames must be {[F, ch, cw]}, got {list(U.shape)} and {list(V.shape)}")
    own = isinstance(dst, (str, os.PathLike))
    f = open(dst, "wb") if own else dst
    try:
        f.write(stream_header(W, H, fps, chroma, full_range))
        for k in range(F):
            f.write(b"FRAME" + frame_fields + b"\n" + Y[k].tobytes())
            if chroma != "mono":
                f.write(U[k].tobytes() + V[k].tobytes())
    finally:
        if own:
            f.close()


# ---- the writer (include/poserisk_hip.h, section j7) ---------------------------------------------------------------------------
def stream_header(W, H, fps=30.0, chroma="420jpeg", full_range=None):
    """The stream header line, its '\\n' included.  fps a number or (num, den); full_range True | False writes XCOLORRANGE, None
    leaves it out."""
    import fractions
    if chroma not in CHROMAS:
        raise ValueError(f"chroma {chroma!r} is not one of {CHROMAS}")
    num, den = fps if isinstance(fps, tuple) else fractions.Fraction(float(fps)).limit_denominator(1001).as_integer_ratio()
    head = f"YUV4MPEG2 W{W} H{H} F{num}:{den} Ip A1:1 C{chroma}"
    if full_range is not None:
        head += " XCOLORRANGE=" + ("FULL" if full_range else "LIMITED")
    return head.encode() + b"\n"


def yuv_enc_plan(matrix, full_range):
    """pr_yuv_enc_plan -> (kyr, kyg, kyb, kc, kur, kug, kvb, kvg, yo)."""
    if matrix not in MATRICES:
        raise ValueError(f"matrix {matrix!r} is not known: '601' or '709'")
    plan = _lib.YuvEncCoeffs()
    _lib.check(_lib.load().pr_yuv_enc_plan(MATRICES[matrix], int(bool(full_range)), C.byref(plan)), "pr_yuv_enc_plan")
    return tuple(getattr(plan, name) for name, _ in _lib.YuvEncCoeffs._fields_)


def encoded_size(W, H, chroma="420mpeg2", pad_even=False):
    """-> (out_W, out_H, bytes a frame takes in the stream: "FRAME\\n" and its planes).  pad_even rounds both sides up to even."""
    if chroma not in CHROMAS:
        raise ValueError(f"chroma {chroma!r} is not one of {CHROMAS}")
    W, H = int(W), int(H)
    ow, oh = (W + (W & 1), H + (H & 1)) if pad_even else (W, H)
    cw = (ow + 1) // 2 if chroma in ("420jpeg", "420mpeg2", "422") else ow
    ch = (oh + 1) // 2 if chroma in ("420jpeg", "420mpeg2") else oh
    return ow, oh, 6 + ow * oh + (0 if chroma == "mono" else 2 * cw * ch)


def encode_frames(frames, chroma="420mpeg2", matrix="601", full_range=False, bgr=False, pad_even=False, out=None):
    """pr_yuv_encode: `frames` u8[F,H,W,3] on the device (RGB; BGR with bgr=True) -> u8[F, 6 + frame_bytes] on the device, the
    frames of a YUV4MPEG2 stream one after the other ("FRAME\\n", Y, U, V), ready to be written behind stream_header(out_W,
    out_H, ...).  pad_even pads odd sides by one replicated row / column (encoded_size gives the sizes).  Asynchronous on the
    current stream; with `out` given it allocates and synchronises nothing."""
    if not (isinstance(frames, torch.Tensor) and frames.is_cuda):
        raise _lib.PoseRiskHipError("encode_frames: the conversion runs on the GPU only (no CPU fallback)")
    if frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[3] != 3 or not frames.is_contiguous():
        raise ValueError(f"encode_frames: frames must be a contiguous uint8 [F,H,W,3] tensor, got {frames.dtype} {tuple(frames.shape)}")
    device, (F, H, W) = frames.device, (int(s) for s in frames.shape[:3])
    ow, oh, size = encoded_size(W, H, chroma, pad_even)
    a = _lib.YuvEncArgs()
    a.plan = _lib.YuvEncCoeffs(*yuv_enc_plan(matrix, full_range))
    a.F, a.H, a.W, a.out_H, a.out_W, a.chroma, a.bgr = F, H, W, oh, ow, CHROMAS.index(chroma), int(bool(bgr))
    with torch.cuda.device(device):
        if out is None:
            out = torch.empty((F, size), dtype=torch.uint8, device=device)
        _check_out(out, (F, size), device, "encode_frames")
        a.src, a.dst = frames.data_ptr(), out.data_ptr()
        _lib.check(_lib.load().pr_yuv_encode(C.byref(a), torch.cuda.current_stream(device).cuda_stream), "pr_yuv_encode")
    return out


class Writer:
    """A YUV4MPEG2 stream of `width` x `height` RGB frames, converted on the GPU (encode_frames), to `dst`: a path, a binary file
    object, "-" (standard output), or -- with dst None and command=[argv] -- a child process fed on its standard input, for
    example ["ffmpeg", "-v", "error", "-y", "-f", "yuv4mpegpipe", "-i", "-", "-c:v", "libx264", "out.mp4"].  The stream header is
    written on construction; .out_width and .out_height are the stream's sides (pad_even rounds odd ones up).

    put(frames) converts a batch, starts its download into one of two pinned buffers and writes the PREVIOUS batch while this
    one converts; close() writes what is left and closes what the writer opened.  Never a shell and never this process's own
    program; a child is reaped whatever happens.  A command that cannot be started, a write that fails with a broken pipe and
    a non-zero exit status raise RuntimeError naming the command, the status and the tail of the child's standard error."""

    def __init__(self, dst=None, width=None, height=None, fps=30.0, chroma="420mpeg2", matrix="601", full_range=False, bgr=False,
                 pad_even=False, command=None):
        if (dst is None) == (command is None):
            raise ValueError("y4m.Writer: give either dst (a path, a binary file object or '-') or command=[argv]")
        if matrix not in MATRICES:
            raise ValueError(f"matrix {matrix!r} is not known: '601' or '709'")
        self.width, self.height = int(width), int(height)
        self.out_width, self.out_height, self.frame_size = encoded_size(self.width, self.height, chroma, pad_even)
        self.chroma, self.matrix, self.full_range, self.bgr, self.pad_even = chroma, matrix, bool(full_range), bool(bgr), bool(pad_even)
        self.frames_written = 0
        self._child = self._f = None
        self._own = self._closed = False
        self._pinned, self._staged, self._pending, self._which = [None, None], None, None, 0
        if command is not None:
            self._child = Child([os.fspath(a) for a in command], "the video encoder", feed=True)
            self._f = self._child.pipe
        elif isinstance(dst, (str, os.PathLike)) and os.fspath(dst) != "-":
            self._f, self._own = open(dst, "wb"), True
        elif isinstance(dst, (str, os.PathLike)):
            self._f = sys.stdout.buffer
        else:
            self._f = dst
        self._write(stream_header(self.out_width, self.out_height, fps, chroma, self.full_range))

    def __enter__(self):
        return self

    def __exit__(self, kind, *exc):
        if kind is None:
            self.close()
        else:
            self.abort()                              # the caller's exception stands; the child is reaped all the same

    def abort(self):
        """Gives up what is queued, closes the sink and reaps a child without raising for its status: for a caller that is
        already handling an error of its own."""
        self._finish(raising=False)

    def _write(self, data):
        try:
            self._f.write(data)
        except (BrokenPipeError, ConnectionResetError) as e:
            if self._child is None:
                raise
            self._finish(failure=f"it closed its standard input after {self.frames_written} frames ({e.strerror or e})")

    def _flush(self):
        if self._pending is not None:
            event, view, frames = self._pending
            self._pending = None
            event.synchronize()
            self._write(memoryview(view))
            self.frames_written += frames

    def put_stream_bytes(self, data, frames=0):
        """Host only: writes `data` (bytes-like: whole frames as encode_frames lays them out) behind what put has queued.
        What put itself ends in, so a test without a GPU drives the same path."""
        if self._closed:
            raise ValueError("y4m.Writer: closed")
        self._flush()
        self._write(memoryview(data))
        self.frames_written += int(frames)

    def put(self, frames):
        """frames u8[F,height,width,3] on the device.  Returns after the PREVIOUS batch's bytes are written; this batch's are
        written by the next put or by close."""
        if self._closed:
            raise ValueError("y4m.Writer: closed")
        if not (isinstance(frames, torch.Tensor) and frames.is_cuda):
            raise _lib.PoseRiskHipError("y4m.Writer.put: the conversion runs on the GPU only (no CPU fallback)")
        if tuple(frames.shape[1:]) != (self.height, self.width, 3):
            raise ValueError(f"y4m.Writer.put: frames must be [F,{self.height},{self.width},3], got {tuple(frames.shape)}")
        F = int(frames.shape[0])
        if F == 0:
            return
        device = frames.device
        with torch.cuda.device(device):
            if self._staged is None or self._staged.shape[0] < F or self._staged.device != device:
                self._staged = torch.empty((F, self.frame_size), dtype=torch.uint8, device=device)
            host = self._pinned[self._which]
            if host is None or host.shape[0] < F:
                host = self._pinned[self._which] = torch.empty((F, self.frame_size), dtype=torch.uint8, pin_memory=True)
            encode_frames(frames.contiguous(), self.chroma, self.matrix, self.full_range, self.bgr, self.pad_even, out=self._staged[:F])
            host[:F].copy_(self._staged[:F], non_blocking=True)
            event = torch.cuda.Event()
            event.record(torch.cuda.current_stream(device))
        self._flush()                                 # the previous batch: written while this one converts and downloads
        self._pending = (event, host[:F].numpy().reshape(-1), F)
        self._which ^= 1

    def close(self):
        """Writes what is left, closes what the writer opened; for a child closes its standard input and waits for it."""
        if self._closed:
            return
        self._flush()
        self._finish()

    def _finish(self, failure=None, raising=True):
        """Closes the sink and reaps the child; raises RuntimeError for a failed child (unless raising is False)."""
        if self._closed:
            return
        self._closed = True
        self._pending = None
        if self._child is None:
            if self._own:
                self._f.close()
            else:
                try:
                    self._f.flush()
                except (AttributeError, ValueError):
                    pass
            return
        try:
            self._f.close()                           # flushes: a child that is gone answers with a broken pipe here too
        except (BrokenPipeError, ConnectionResetError) as e:
            failure = failure or f"it closed its standard input after {self.frames_written} frames ({e.strerror or e})"
        except OSError:
            pass
        self._child.finish(5 if failure is not None or not raising else 600, failure, raising)
