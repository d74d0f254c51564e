"""What jpeg.py, png.py, y4m.py and frontend.py share around their kernels: the device they run on, the plans they upload once,
the files they read into pinned memory, and the encoders' files brought to the host."""
import os

import numpy as np
import torch

from . import _lib


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
