"""REBA's activity score and RULA's muscle use derived from each track's motion on the GPU (pr_activity_tracks; the contract
is section t1 of include/poserisk_hip.h, tests/activity_ref.py restates it in numpy).

The worksheets add +1 where a body part is held for longer than a minute, +1 for small actions repeated more than four times a
minute, +1 for rapid large changes of posture (REBA), and +1 muscle use to a group that is mainly static for over a minute or
repeated four times a minute (RULA).  The reference takes these as constants of the information file; here they follow from the
rotations of the twelve joints the rules read, row by row, and are ADDED to those constants (leave them at 0).  What "held",
"an action" and "a large change" mean in degrees is this project's choice -- the worksheets give no angles -- and nobody has
measured the rule on real footage.  There is no CPU path."""
import ctypes as C
import math

import numpy as np
import torch

from . import _lib

MAX_HOLD_FRAMES = 16384
JOINT_NAMES = ("Torso", "Neck", "L_Knee", "R_Knee", "L_Thorax", "L_Shoulder", "L_Elbow", "L_Wrist", "R_Thorax", "R_Shoulder",
               "R_Elbow", "R_Wrist")          # bit b of every mask
KINDS = ("held", "repeated", "rapid", "moved")                # the columns of flags
ADDS = ("reba_activity", "a_muscle_l", "a_muscle_r", "b_muscle")   # the columns of adds
# cfg.ACTIVITY's defaults; the degrees are this project's choice, the worksheets give none
DEFAULTS = dict(derive=False, hold_seconds=60.0, static_deg=10.0, move_deg=15.0, rep_events=8, rapid_seconds=1.0, rapid_deg=45.0,
                gap_seconds=0.2)


def frames(seconds, fps):
    """max(1, ceil(seconds * fps)): a duration in frames."""
    return max(1, int(math.ceil(float(seconds) * float(fps))))


def thresholds(static_deg, move_deg, rapid_deg):
    """Degrees -> (dot_static, dot_move, dot_rapid) = 1 + 2 cos(angle): the trace of the relative rotation at that angle."""
    return tuple(1.0 + 2.0 * math.cos(math.radians(float(d))) for d in (static_deg, move_deg, rapid_deg))


def check_parameters(fps, hold_seconds=60.0, static_deg=10.0, move_deg=15.0, rep_events=8, rapid_seconds=1.0, rapid_deg=45.0,
                     gap_seconds=0.2, **unknown):
    """-> dict(fps, the seconds and degrees as given, hold_frames, rapid_frames, gap_frames, rep_events, dot_static, dot_move,
    dot_rapid), or ValueError by name; no device call."""
    unknown.pop("derive", None)
    if unknown:
        raise ValueError(f"activity: unknown parameter(s) {sorted(unknown)} (cfg.ACTIVITY holds {sorted(DEFAULTS)})")
    if fps is None:
        raise ValueError("activity: fps is needed to turn hold_seconds, rapid_seconds and gap_seconds into frames, and none was given")
    nums = dict(fps=fps, hold_seconds=hold_seconds, rapid_seconds=rapid_seconds, gap_seconds=gap_seconds, static_deg=static_deg,
                move_deg=move_deg, rapid_deg=rapid_deg)
    for name, v in nums.items():
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not math.isfinite(float(v)):
            raise ValueError(f"activity: {name} = {v!r} is not a finite number")
        nums[name] = float(v)
    for name in ("fps", "hold_seconds", "rapid_seconds", "gap_seconds"):
        if nums[name] <= 0.0:
            raise ValueError(f"activity: {name} = {nums[name]} is not positive")
    for name in ("static_deg", "move_deg", "rapid_deg"):
        if not 0.0 <= nums[name] <= 180.0:
            raise ValueError(f"activity: {name} = {nums[name]} outside 0..180 degrees")
    if isinstance(rep_events, bool) or int(rep_events) != rep_events or int(rep_events) < 0:
        raise ValueError(f"activity: rep_events = {rep_events!r} is not an integer >= 0")
    H, R, G = (frames(nums[k], nums["fps"]) for k in ("hold_seconds", "rapid_seconds", "gap_seconds"))
    if H > MAX_HOLD_FRAMES:
        raise ValueError(f"activity: hold_seconds = {nums['hold_seconds']} at {nums['fps']} fps is {H} frames, more than {MAX_HOLD_FRAMES}")
    if R > H:
        raise ValueError(f"activity: rapid_seconds = {nums['rapid_seconds']} ({R} frames) is longer than hold_seconds = "
                         f"{nums['hold_seconds']} ({H} frames)")
    ds, dm, dr = thresholds(nums["static_deg"], nums["move_deg"], nums["rapid_deg"])
    return dict(nums, rep_events=int(rep_events), hold_frames=H, rapid_frames=R, gap_frames=G, dot_static=ds, dot_move=dm, dot_rapid=dr)


def activity_tracks(rotmat, frame_no, track_start, fps, **parameters):
    """rotmat f32[N,24,3,3] (CUDA), frame_no int[N] (tensor or array: each row's frame number), track_start int[T+1] (host:
    track t owns rows track_start[t] .. track_start[t+1] - 1), fps, and cfg.ACTIVITY's parameters by keyword ->
    dict(flags i32[N,4]: the held, repeated, rapid and moved masks (bit b = JOINT_NAMES[b]); adds i32[N,4]: reba_activity,
    a_muscle_l, a_muscle_r, b_muscle; parameters: check_parameters' dict, seconds and frames).
    Every argument is checked before any device call; the inputs are not written."""
    par = check_parameters(fps, **parameters)
    if not isinstance(rotmat, torch.Tensor):
        raise TypeError(f"activity_tracks: rotmat must be a torch tensor on the GPU, not {type(rotmat).__name__}")
    if rotmat.dtype != torch.float32 or rotmat.dim() != 4 or tuple(rotmat.shape[1:]) != (24, 3, 3):
        raise ValueError(f"activity_tracks: rotmat must be float32[N,24,3,3], got {rotmat.dtype} {tuple(rotmat.shape)}")
    dev, N = rotmat.device, int(rotmat.shape[0])
    ts = np.asarray(track_start)
    if ts.ndim != 1 or ts.size < 1 or ts.dtype.kind not in "iu":
        raise ValueError("activity_tracks: track_start must be a 1-D integer array of T + 1 row offsets")
    ts = ts.astype(np.int64)
    if ts[0] != 0 or ts[-1] != N or np.any(np.diff(ts) < 0):
        raise ValueError(f"activity_tracks: track_start must run 0 = s_0 <= s_1 <= ... <= s_T = N = {N}, got {ts[:8].tolist()}"
                         f"{'...' if ts.size > 8 else ''}")
    if isinstance(frame_no, torch.Tensor):
        if frame_no.dtype not in (torch.int32, torch.int64) or frame_no.dim() != 1:
            raise ValueError("activity_tracks: frame_no must be a 1-D integer tensor")
        fno_host = None
    else:
        fno_host = np.asarray(frame_no)
        if fno_host.ndim != 1 or fno_host.dtype.kind not in "iu":
            raise ValueError("activity_tracks: frame_no must be a 1-D integer array")
    if (frame_no.shape[0] if fno_host is None else fno_host.shape[0]) != N:
        raise ValueError(f"activity_tracks: frame_no has {len(frame_no)} entries, rotmat {N} rows")
    if fno_host is not None and N and (fno_host.min() < -2 ** 31 or fno_host.max() >= 2 ** 31):
        raise ValueError("activity_tracks: frame_no does not fit int32")
    if dev.type != "cuda":
        raise _lib.PoseRiskHipError("activity_tracks: the tensors must be on the GPU (no CPU fallback)")
    # ---- device work from here
    lib = _lib.load()
    rotmat = rotmat.contiguous()
    fno = frame_no.to(dev, torch.int32).contiguous() if fno_host is None else torch.as_tensor(fno_host.astype(np.int32), device=dev)
    flags = torch.empty((N, 4), dtype=torch.int32, device=dev)
    adds = torch.empty((N, 4), dtype=torch.int32, device=dev)
    ws = torch.empty((max(int(lib.pr_activity_workspace_bytes(N)), 4),), dtype=torch.uint8, device=dev)
    ptr = lambda t: t.data_ptr() if t.numel() else None      # (a tensor without elements has no storage: N = 0 passes nulls)
    params = _lib.ActivityParams(par["hold_frames"], par["rapid_frames"], par["gap_frames"], par["rep_events"], par["dot_static"],
                                 par["dot_move"], par["dot_rapid"])
    starts = (C.c_int * ts.size)(*ts.tolist())
    _lib.check(lib.pr_activity_tracks(C.byref(params), ptr(rotmat), ptr(fno), starts, ts.size - 1, N, ptr(flags), ptr(adds), ws.data_ptr(),
                                      torch.cuda.current_stream(dev).cuda_stream), "pr_activity_tracks")
    return dict(flags=flags, adds=adds, parameters=par)


def counts(flags):
    """Host array i32[n,4] of one person -> {kind: {'rows': the rows with any bit of that mask, 'joints': {name: rows with that
    joint's bit}}} for held, repeated, rapid and moved."""
    flags = np.asarray(flags).reshape(-1, 4)
    out = {}
    for c, kind in enumerate(KINDS):
        col = flags[:, c]
        out[kind] = dict(rows=int(np.count_nonzero(col)), joints={name: int(np.count_nonzero(col >> b & 1)) for b, name in enumerate(JOINT_NAMES)})
    return out
