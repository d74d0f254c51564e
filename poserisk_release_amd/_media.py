"""What jpeg.py, png.py, y4m.py and frontend.py share around their kernels: the device they run on, the plans they upload once,
the files they read into pinned memory, and the encoders' files brought to the host.

`decode_chunks` is the one loop under jpeg.decode_files and png.decode_files: per chunk ONE pinned buffer (`layout`), ONE upload,
one decode call; the rules about the lifetime of buffer, device copy and workspace are there and nowhere else."""
import os
import types

import numpy as np
import torch

from . import _lib

PR_ERR_CAPACITY = -4   # include/poserisk_hip.h: an array of the caller's is too short; the parsers' counts say what is needed


def cuda_device(device, who, what):
    """`device` as a CUDA device with an index; anything else raises: "<who>: <what> on the GPU only (no CPU fallback)"."""
    device = torch.device(device)
    if device.type != "cuda":
        raise _lib.PoseRiskHipError(f"{who}: {what} on the GPU only (no CPU fallback)")
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    return device


_plans = {}


def device_plan(key, device, make):
    """The plan of the parameter set `key` (its first item names the kind of plan) on `device` -> (u8 tensor on the device, what
    else `make` returned): made once, kept.  `make()` is the host half -> (the plan's bytes, anything to keep beside them).  The
    first call of a parameter set copies the plan from pageable host memory and waits for the copy, so that every stream, then
    and later, finds the plan complete; every further call only looks it up."""
    plan = _plans.get((key, device))
    if plan is None:
        data, extra = make()
        tensor = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).to(device)
        torch.cuda.current_stream(device).synchronize()
        plan = _plans[(key, device)] = (tensor, extra)
    return plan


def align(n, a=256):
    return (n + a - 1) // a * a


def size(p):   # the bytes of an item: a path's file size, or the length of a bytes object
    return os.path.getsize(p) if isinstance(p, (str, os.PathLike)) else len(p)


def blob(p):   # an item (a path, or a bytes object) as bytes
    return open(p, "rb").read() if isinstance(p, (str, os.PathLike)) else bytes(p)


def pack(blobs):
    """A list of bytes objects as the parsers take it -> (offsets int64[F + 1], the bytes joined as uint8; \0 for an empty list)."""
    offsets = np.zeros(len(blobs) + 1, np.int64)
    np.cumsum([len(b) for b in blobs], out=offsets[1:])
    return offsets, np.frombuffer(b"".join(bytes(b) for b in blobs) or b"\0", np.uint8)


def layout(total, arrays):
    """The descriptor arrays [(itemsize, count), ...] behind `total` bytes of files in one buffer -> ([offset of each], the buffer's
    size): each begins at the next multiple of 256 behind the end of what precedes it, the first behind at least one byte."""
    at, end = [], max(total, 1)
    for itemsize, count in arrays:
        at.append(align(end))
        end = at[-1] + itemsize * count
    return at, end


def decode_chunks(items, device, out, *, cut, itemsizes, rooms, regrow, parse, parser, used, sized, decode, refusal_name, refused):
    """The loop under jpeg.decode_files and png.decode_files -> (frames u8[F,H,W,3], status int32[F]) on `device`; `out` is None or
    the caller's frames.  Per chunk the host waits until the previous chunk's upload (not its decode) has left the pinned buffer,
    reads the files into it, parses -- after PR_ERR_CAPACITY again where the bytes lie, in a larger buffer if need be --, uploads
    the used part with one asynchronous copy and enqueues the decode.  The first accepted frame fixes (H, W): frames of chunks
    before it are zero with status `refused`, and such a chunk uploads and launches nothing.  The format gives
      cut(lo)                  the byte sizes of the files of the chunk that begins at item lo (at least one)
      itemsizes                the entry size of each descriptor array, in the order the arrays lie behind the files' bytes
      rooms(n)                 the entries each array gets in a chunk of n files
      regrow(n, room, counts)  the same after the parser answered PR_ERR_CAPACITY with `counts` to `room`
      parse(data, offsets, H, W, views, pstatus) -> (rc, counts)   the host parser (`parser`: its name) writing into `views`, the
                               arrays as uint8 views of the buffer; counts[2:4] is the (H, W) it fixed, or 0
      used                     the index in counts of the filled entries of the LAST array: the upload ends behind them
      sized(H, W)              called once, where `status` is made
      decode(c) -> (workspace bytes, call)   c: lo, n, total, H, W, counts, pstatus, views, and on the device base, at (the arrays'
                               offsets from base), out, status (the chunk's slices); call(workspace, its size, stream) enqueues
      refusal_name, refused    the words of a parse status; the status of a refused frame"""
    F, H, W, lo = len(items), 0, 0, 0
    frames = status = pinned = ws = uploaded = first_refusal = None
    with torch.cuda.device(device):
        stream = torch.cuda.current_stream(device)
        while lo < F:
            sizes = cut(lo)
            n = len(sizes)
            offsets = np.zeros(n + 1, np.int64)
            np.cumsum(sizes, out=offsets[1:])
            total, room, pst, read = int(offsets[-1]), rooms(n), np.zeros(n, np.int32), False
            if uploaded is not None:
                uploaded.synchronize()                           # the previous chunk has left the buffer
            while True:
                at, end = layout(total, list(zip(itemsizes, room)))
                if pinned is None or pinned.numel() < end:
                    grown = torch.empty(end, dtype=torch.uint8).pin_memory()
                    if read:
                        grown[:total] = pinned[:total]           # the files' bytes move with the parse that outgrew the buffer
                    pinned = grown
                host = pinned.numpy()
                if not read:
                    read_files(host, items[lo:lo + n], offsets)
                    read = True
                views = [host[o:o + s * k] for o, s, k in zip(at, itemsizes, room)]
                rc, counts = parse(host[:max(total, 1)], offsets, H, W, views, pst)
                if rc != PR_ERR_CAPACITY:
                    _lib.check(rc, parser)
                    break
                room = regrow(n, room, counts)                   # parse again where the bytes lie
            if H == 0 and pst.any() and first_refusal is None:
                first_refusal = (lo + int(np.nonzero(pst)[0][0]), refusal_name(pst[np.nonzero(pst)[0][0]]))
            if H == 0 and counts[2]:
                H, W = int(counts[2]), int(counts[3])
                frames = out if out is not None else torch.empty((F, H, W, 3), dtype=torch.uint8, device=device)
                if tuple(frames.shape) != (F, H, W, 3) or frames.dtype != torch.uint8 or not frames.is_contiguous() \
                        or frames.device != device:
                    raise ValueError(f"out must be a contiguous uint8 {[F, H, W, 3]} tensor on {device}")
                status = torch.full((F,), refused, dtype=torch.int32, device=device)   # chunks before the first size
                sized(H, W)
                frames[:lo].zero_()
            if H != 0:                                           # else nothing accepted so far: no size to decode at
                nbytes = at[-1] + int(counts[used]) * itemsizes[-1]
                dev = torch.empty(nbytes, dtype=torch.uint8, device=device)
                dev.copy_(pinned[:nbytes], non_blocking=True)    # the chunk's one upload
                uploaded = torch.cuda.Event()
                uploaded.record(stream)
                need, call = decode(types.SimpleNamespace(lo=lo, n=n, total=total, H=H, W=W, counts=counts, pstatus=pst, views=views,
                                                          base=dev.data_ptr(), at=at, out=frames[lo:lo + n].data_ptr(),
                                                          status=status[lo:lo + n].data_ptr()))
                if ws is None or ws.numel() < need:
                    ws = torch.empty(need, dtype=torch.uint8, device=device)
                call(ws.data_ptr(), ws.numel(), stream.cuda_stream)
                for t in (dev, ws):
                    t.record_stream(stream)
            lo += n
        if uploaded is not None:
            uploaded.synchronize()
    if frames is None:
        if first_refusal:
            raise _lib.PoseRiskHipError(f"decode_files: no frame was accepted; frame {first_refusal[0]}: {first_refusal[1]}")
        frames = torch.empty((0, 0, 0, 3), dtype=torch.uint8, device=device)
        status = torch.zeros(0, dtype=torch.int32, device=device)
    return frames, status


def bad_frames(items, status, status_text, parse, refusal_name, refused):
    """[(frame index, reason)] for every frame of a decode_files call whose status is non-zero (one device -> host copy): the
    module's `status_text`, and for a frame with the `refused` bit what the module's `parse` says of its file alone."""
    items, st, out = list(items), status.cpu().numpy(), []
    for i in np.nonzero(st)[0]:
        why = status_text(int(st[i]))
        if st[i] & refused:
            _, _, _, pst, h, w, *_ = parse([blob(items[i])])
            why = refusal_name(pst[0]) if pst[0] else f"its size {w}x{h} differs from the other frames of the call"
        out.append((int(i), why))
    return out


def read_files(host, items, offsets):
    """Item i (a path, or a bytes object) into host[offsets[i]:offsets[i + 1]] (`host`: a uint8 array over the pinned buffer).
    A file that no longer has the size `offsets` was made from raises OSError."""
    for p, a, b in zip(items, offsets[:-1], offsets[1:]):
        if isinstance(p, (str, os.PathLike)):
            with open(p, "rb") as f:
                got = f.readinto(memoryview(host[a:b]))
            if got != b - a:
                raise OSError(f"{p!r} changed size while it was read")
        else:
            host[a:b] = np.frombuffer(bytes(p), np.uint8)


def download_files(buffer, nbytes):
    """[bytes] of an encode_frames result; only the used bytes cross to the host: the sizes first (one small copy), then the
    slices buffer[f, :nbytes[f]] packed into one device tensor and copied once."""
    n = nbytes.cpu().numpy().astype(np.int64)
    if n.size == 0:
        return []
    packed = torch.cat([buffer[f, :k] for f, k in enumerate(n.tolist())]).cpu().numpy().tobytes()
    ends = np.cumsum(n)
    return [packed[e - k:e] for e, k in zip(ends, n)]


def encode_files(encode, images, first, bound, name="encode_frames"):
    """The files of `images` u8[b,H,W,3] as [bytes].  `encode(images, capacity)` is an encode_frames call -> (buffer, nbytes, status):
    the batch goes into slots of `first` bytes (None: the encoder's default), and a frame that overflowed its slot (ENC_ST_OVERFLOW,
    the only status an encoder gives) is encoded again alone with `bound`, the slot no file exceeds.  A file depends neither on its
    slot nor on its neighbours.  A frame that still does not fit raises RuntimeError beginning with `name`."""
    buf, nbytes, status = encode(images, first)
    files = download_files(buf, nbytes)
    for i in np.nonzero(status.cpu().numpy())[0]:
        buf1, nbytes1, status1 = encode(images[i:i + 1], bound)
        if int(status1[0]):
            raise RuntimeError(f"{name}: status {int(status1[0])} for a frame with the largest slot")
        files[i] = download_files(buf1, nbytes1)[0]
    return files
