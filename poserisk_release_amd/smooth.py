"""Temporal smoothing of each track's poses on the GPU (pr_smooth_tracks; the contract is section s1 of
include/poserisk_hip.h, tests/smooth_ref.py restates it in numpy).

Stage 1 replaces every joint rotation (and cam, betas) by the medoid of its window of `median_radius` frames, which removes
single-frame outliers; stage 2 averages with Gaussian weights of `sigma` frames and projects each joint back onto the nearest
rotation, which removes jitter.  Both units are FRAMES, not seconds.  Windows are defined on frame numbers and never cross a
track boundary.  There is no CPU path."""
import ctypes as C
import math

import numpy as np
import torch

from . import _lib

MAX_RADIUS = 15


def gaussian_radius(sigma):
    """g = min(ceil(3 sigma), 15): the radius of stage 2's window, in frames."""
    return int(min(math.ceil(3.0 * sigma), MAX_RADIUS)) if sigma > 0 else 0


def check_parameters(median_radius, sigma):
    """-> (int m, float sigma), or ValueError by name; no device call."""
    if isinstance(median_radius, bool) or int(median_radius) != median_radius:
        raise ValueError(f"smooth: median_radius = {median_radius!r} is not an integer (the unit is frames)")
    if not 0 <= int(median_radius) <= MAX_RADIUS:
        raise ValueError(f"smooth: median_radius = {median_radius} outside 0..{MAX_RADIUS} frames")
    sigma = float(sigma)
    if not (math.isfinite(sigma) and sigma >= 0.0):
        raise ValueError(f"smooth: sigma = {sigma} is not a finite number of frames >= 0")
    return int(median_radius), sigma


def _tensor(t, name, tail, device):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"smooth_tracks: {name} must be a torch tensor on the GPU, not {type(t).__name__}")
    if device is not None and t.device != device:
        raise ValueError(f"smooth_tracks: {name} is on {t.device}, rotmat on {device}")
    if t.dtype != torch.float32 or t.dim() != 1 + len(tail) or tuple(t.shape[1:]) != tail:
        raise ValueError(f"smooth_tracks: {name} must be float32[N,{','.join(map(str, tail))}], got {t.dtype} {tuple(t.shape)}")
    return t


def smooth_tracks(rotmat, frame_no, track_start, median_radius, sigma, betas=None, cam=None):
    """rotmat f32[N,24,3,3] (CUDA), frame_no int[N] (tensor or array: each row's frame number), track_start int[T+1] (host:
    track t owns rows track_start[t] .. track_start[t+1] - 1; 0 = s_0 <= ... <= s_T = N), median_radius 0..15 and sigma >= 0 in
    frames, optionally betas f32[N,10] and cam f32[N,3] ->
    dict(rotmat, betas, cam (None where not given), status i32[N]: bit j = joint j kept stage 1's value because its window's
    rotations disagree too much to average, replaced i32[N]: bit j = stage 1 took joint j (24: cam, 25: betas) from another row).
    Every argument is checked before any device call; the inputs are not written."""
    m, sigma = check_parameters(median_radius, sigma)
    rotmat = _tensor(rotmat, "rotmat", (24, 3, 3), None)
    dev, N = rotmat.device, int(rotmat.shape[0])
    betas = _tensor(betas, "betas", (10,), dev) if betas is not None else None
    cam = _tensor(cam, "cam", (3,), dev) if cam is not None else None
    for name, t in (("betas", betas), ("cam", cam)):
        if t is not None and t.shape[0] != N:
            raise ValueError(f"smooth_tracks: {name} has {t.shape[0]} rows, rotmat {N}")
    ts = np.asarray(track_start)
    if ts.ndim != 1 or ts.size < 1 or ts.dtype.kind not in "iu":
        raise ValueError("smooth_tracks: track_start must be a 1-D integer array of T + 1 row offsets")
    ts = ts.astype(np.int64)
    if ts[0] != 0 or ts[-1] != N or np.any(np.diff(ts) < 0):
        raise ValueError(f"smooth_tracks: track_start must run 0 = s_0 <= s_1 <= ... <= s_T = N = {N}, got {ts[:8].tolist()}"
                         f"{'...' if ts.size > 8 else ''}")
    if isinstance(frame_no, torch.Tensor):
        if frame_no.dtype not in (torch.int32, torch.int64) or frame_no.dim() != 1:
            raise ValueError("smooth_tracks: frame_no must be a 1-D integer tensor")
        fno_host = None
    else:
        fno_host = np.asarray(frame_no)
        if fno_host.ndim != 1 or fno_host.dtype.kind not in "iu":
            raise ValueError("smooth_tracks: frame_no must be a 1-D integer array")
    if (frame_no.shape[0] if fno_host is None else fno_host.shape[0]) != N:
        raise ValueError(f"smooth_tracks: frame_no has {len(frame_no)} entries, rotmat {N} rows")
    if fno_host is not None and N and (fno_host.min() < -2 ** 31 or fno_host.max() >= 2 ** 31):
        raise ValueError("smooth_tracks: frame_no does not fit int32")
    if dev.type != "cuda":
        raise _lib.PoseRiskHipError("smooth_tracks: the tensors must be on the GPU (no CPU fallback)")
    # ---- device work from here
    lib = _lib.load()
    rotmat, betas, cam = (t.contiguous() if t is not None else None for t in (rotmat, betas, cam))
    if fno_host is None:
        fno = frame_no.to(dev, torch.int32).contiguous()
    else:
        fno = torch.as_tensor(fno_host.astype(np.int32), device=dev)
    out = dict(rotmat=torch.empty_like(rotmat), betas=torch.empty_like(betas) if betas is not None else None,
               cam=torch.empty_like(cam) if cam is not None else None,
               status=torch.empty((N,), dtype=torch.int32, device=dev), replaced=torch.empty((N,), dtype=torch.int32, device=dev))
    ws = None
    if m > 0 and sigma > 0:
        ws = torch.empty((max(int(lib.pr_smooth_workspace_bytes(N, betas is not None, cam is not None)), 4),), dtype=torch.uint8, device=dev)
    ptr = lambda t: t.data_ptr() if t is not None and t.numel() else None
    # (a tensor without elements has no storage: N = 0 passes null pointers, which the entry accepts)
    params = _lib.SmoothParams(m, 0, sigma)
    ins = _lib.SmoothInputs(ptr(rotmat), ptr(betas), ptr(cam))
    outs = _lib.SmoothOutputs(ptr(out["rotmat"]), ptr(out["betas"]), ptr(out["cam"]), ptr(out["replaced"]))
    starts = (C.c_int * ts.size)(*ts.tolist())
    _lib.check(lib.pr_smooth_tracks(C.byref(params), C.byref(ins), ptr(fno), starts, ts.size - 1, N, C.byref(outs),
                                    ptr(out["status"]), ptr(ws), torch.cuda.current_stream(dev).cuda_stream), "pr_smooth_tracks")
    return out


def counts(status, replaced):
    """Host arrays i32[n] of one person -> (the (row, joint) items stage 1 replaced, the (row, joint) fallbacks of stage 2)."""
    joints = np.uint32((1 << 24) - 1)
    pop = lambda a: int(sum(bin(int(v)).count("1") for v in (np.asarray(a).astype(np.uint32) & joints)))
    return pop(replaced), pop(status)
