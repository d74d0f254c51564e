"""Mesh overlay: the fitted SMPL mesh of every scored crop drawn over its video frame, one colour per body part by risk
level (include/poserisk_hip.h, pr_render_overlay; the kernels are csrc/render.hip).

`overlay` is the torch wrapper of the kernel.  `face_parts` and `part_colours` turn SMPL's skinning weights and the REBA /
RULA logs into the kernel's face_part and part_rgb tables.  The Predictor's `render_overlay` (dropin/core/outputs.py) chains
them on the arrays `score_frames` returns.

`overlay_people` is the wrapper of pr_render_people (header section r4): the meshes of everybody in a frame on one canvas,
depth-tested against each other; `people_z_step` is the host rule that orders them in depth.  The Predictor's `render_people`
chains them on what `score_people` returns."""
import numpy as np
import torch

from . import _lib

# The parts a face can belong to, in this order for both schemes (face_part values index it).
PARTS = ("trunk", "neck", "leg", "upper_arm_l", "upper_arm_r", "lower_arm_l", "lower_arm_r", "wrist_l", "wrist_r")
# SMPL joint -> part: the joint whose rotation moves that segment (csrc/frame_kernels.hip reads L_SHOULDER = 16 for upper
# arm L, L_ELBOW = 18 for lower arm L, L_WRIST = 20 for wrist L; the hands 22 / 23 follow their wrists).
_JOINT_PART = {0: 0, 3: 0, 6: 0, 9: 0, 13: 0, 14: 0,
               12: 1, 15: 1,
               1: 2, 2: 2, 4: 2, 5: 2, 7: 2, 8: 2, 10: 2, 11: 2,
               16: 3, 17: 4, 18: 5, 19: 6, 20: 7, 22: 7, 21: 8, 23: 8}
JOINT_PART = np.array([_JOINT_PART[j] for j in range(24)], np.int32)
# the log column of each part: REBA int32[N,10] score, trunk, neck, leg, upper_arm L,R, lower_arm L,R, wrist L,R;
# RULA int32[N,12] score, upper_arm L,R, lower_arm L,R, wrist L,R, wrist_twist L,R, neck, trunk, leg.  RULA's wrist-twist
# columns (7, 8) have no segment of their own and are not drawn.
LOG_COLUMNS = {"REBA": (1, 2, 3, 4, 5, 6, 7, 8, 9), "RULA": (10, 9, 11, 1, 2, 3, 4, 5, 6)}
# risk level clip(sub_score - 1, 0, 3): green, yellow, orange, red (RGB)
LEVEL_RGB = np.array([[40, 200, 60], [250, 220, 40], [250, 140, 20], [230, 30, 30]], np.uint8)
NEUTRAL_RGB = np.array([200, 200, 210], np.uint8)


def _scheme(scheme):
    if scheme is None:
        return None
    s = str(scheme).upper()
    if s not in LOG_COLUMNS:
        raise ValueError(f"scheme must be 'REBA', 'RULA' or None, got {scheme!r}")
    return s


def face_parts(weights, faces, scheme=None):
    """Skinning weights f32[V,24] + faces int[F,3] -> int32[F] part index into PARTS: the joint with the largest sum of the
    face's three vertices' weights, mapped by JOINT_PART.  scheme None: one neutral part (all zeros)."""
    faces = np.asarray(faces, np.int64)
    if _scheme(scheme) is None:
        return np.zeros(faces.shape[0], np.int32)
    w = np.asarray(weights, np.float64)
    joint = np.argmax(w[faces[:, 0]] + w[faces[:, 1]] + w[faces[:, 2]], axis=1)
    return JOINT_PART[joint]


def part_colours(logs, scheme=None):
    """REBA int32[N,10] / RULA int32[N,12] logs -> part_rgb u8[N,len(PARTS),3] by risk level; scheme None: u8[N,1,3]
    neutral grey."""
    logs = np.asarray(logs)
    s = _scheme(scheme)
    if s is None:
        return np.broadcast_to(NEUTRAL_RGB, (logs.shape[0], 1, 3)).copy()
    want = 10 if s == "REBA" else 12
    if logs.ndim != 2 or logs.shape[1] != want:
        raise ValueError(f"{s} logs must be int[N,{want}], got shape {logs.shape}")
    level = np.clip(logs[:, list(LOG_COLUMNS[s])].astype(np.int64) - 1, 0, 3)
    return LEVEL_RGB[level]


def _dev_tensor(x, dtype, dev, shape=None, what=""):
    t = torch.as_tensor(x).to(device=dev, dtype=dtype).contiguous()
    if shape is not None and (t.dim() != len(shape) or any(s is not None and t.shape[i] != s for i, s in enumerate(shape))):
        raise ValueError(f"{what} must have shape {shape}, got {tuple(t.shape)}")
    return t


def _host_faces(faces, V):
    """faces int[F,3] as a host array, its indices checked against [0, V): once, here, for both wrappers."""
    faces_host = faces.detach().cpu().numpy() if isinstance(faces, torch.Tensor) else np.asarray(faces)
    if faces_host.ndim != 2 or faces_host.shape[1] != 3 or faces_host.shape[0] == 0:
        raise ValueError(f"faces must be int [F,3], got shape {faces_host.shape}")
    if int(faces_host.min()) < 0 or int(faces_host.max()) >= V:
        raise ValueError(f"face indices {int(faces_host.min())}..{int(faces_host.max())} outside [0, {V})")
    return faces_host


def _mesh_tensors(faces, faces_host, cam, bboxes, face_part, part_rgb, N, dev, min_parts):
    """What both entries read beside the vertices, on `dev` in the kernel's dtypes: faces, cam [N,3], bboxes [N,4], face_part
    [F] (None: all part 0) and part_rgb [N,P,3], P >= min_parts ([P,3]: the same for every mesh; None: neutral grey)."""
    F = faces_host.shape[0]
    f = _dev_tensor(faces if isinstance(faces, torch.Tensor) else faces_host, torch.int32, dev)
    c = _dev_tensor(cam, torch.float32, dev, (N, 3), "cam")
    bb = _dev_tensor(bboxes, torch.float32, dev, (N, 4), "bboxes")
    fp = _dev_tensor(np.zeros(F, np.int32) if face_part is None else face_part, torch.int32, dev, (F,), "face_part")
    rgb = _dev_tensor(NEUTRAL_RGB[None] if part_rgb is None else part_rgb, torch.uint8, dev)
    if rgb.dim() == 2:
        rgb = rgb[None].expand(N, -1, -1).contiguous()
    if rgb.dim() != 3 or rgb.shape[0] != N or rgb.shape[2] != 3 or rgb.shape[1] < min_parts:
        raise ValueError(f"part_rgb must be u8[N,P,3] or u8[P,3], got {tuple(rgb.shape)}")
    return f, c, bb, fp, rgb


def _outputs(out, images, lead, N, V, H, W, dev, return_face_id, return_vert_fx, return_status):
    """out u8[images,H,W,3] (checked when given; `lead` names its first axis) and the optional face_id, vert_fx and status."""
    if out is None:
        out = torch.empty((images, H, W, 3), dtype=torch.uint8, device=dev)
    elif out.shape != (images, H, W, 3) or out.dtype != torch.uint8 or not out.is_contiguous() or out.device != dev:
        raise ValueError(f"out must be a contiguous uint8 [{lead},H,W,3] tensor on the frames' device")
    fid = torch.empty((images, H, W), dtype=torch.int32, device=dev) if return_face_id else None
    vfx = torch.empty((N, V, 4), dtype=torch.int32, device=dev) if return_vert_fx else None
    st = torch.empty((N,), dtype=torch.int32, device=dev) if return_status else None
    return out, fid, vfx, st


def _ptr(t):
    return t.data_ptr() if t is not None else None


def overlay(frames, verts, faces, cam, bboxes, scale=1.2, frame_idx=None, face_part=None, part_rgb=None, alpha=0.6,
            bgr=False, out=None, return_face_id=False, return_vert_fx=False, return_status=False):
    """Draw the meshes over their frames on the GPU.

    frames u8[n_frames,H,W,3] CUDA; verts f32[N,V,3] (SPIN camera axes, metres); faces int[F,3]; cam f32[N,3] (s, tx, ty);
    bboxes f32[N,4] (cx, cy, w, h); scale = cfg.DATASET.bbox_scale; frame_idx int[N] or None (crop n over frame n);
    face_part int[F] or None (all part 0); part_rgb u8[N,P,3] or u8[P,3] (RGB) or None (neutral grey); alpha in [0, 1];
    bgr: the frames' channel order.  Returns out u8[N,H,W,3], followed by face_id int32[N,H,W], vert_fx int32[N,V,4] and
    status int32[N] as asked for.  Face indices are checked here, once, on the host."""
    if not (isinstance(frames, torch.Tensor) and frames.device.type == "cuda"):
        raise _lib.PoseRiskHipError("overlay: frames must be a CUDA tensor (no CPU fallback)")
    if frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[3] != 3:
        raise ValueError("frames must be uint8 [n_frames,H,W,3]")
    dev = frames.device
    frames = frames.contiguous()
    n_frames, H, W, _ = frames.shape
    v = _dev_tensor(verts, torch.float32, dev, (None, None, 3), "verts")
    N, V = v.shape[0], v.shape[1]
    faces_host = _host_faces(faces, V)
    F = faces_host.shape[0]
    f, c, bb, fp, rgb = _mesh_tensors(faces, faces_host, cam, bboxes, face_part, part_rgb, N, dev, min_parts=0)
    idx = None if frame_idx is None else _dev_tensor(frame_idx, torch.int32, dev, (N,), "frame_idx")
    out, fid, vfx, st = _outputs(out, N, "N", N, V, H, W, dev, return_face_id, return_vert_fx, return_status)
    lib = _lib.load()
    nbytes = lib.pr_render_workspace_bytes(N, V, F, H, W)
    ws = torch.empty((max(int(nbytes), 1),), dtype=torch.uint8, device=dev)
    args = _lib.RenderArgs(v.data_ptr(), f.data_ptr(), c.data_ptr(), bb.data_ptr(), frames.data_ptr(), _ptr(idx),
                           fp.data_ptr(), rgb.data_ptr(), out.data_ptr(), _ptr(fid), _ptr(vfx), _ptr(st),
                           N, V, F, rgb.shape[1], n_frames, H, W, int(bool(bgr)), float(scale), float(alpha))
    _lib.check(lib.pr_render_overlay(args, ws.data_ptr(), nbytes, torch.cuda.current_stream(dev).cuda_stream),
               "pr_render_overlay")
    extra = [t for t in (fid, vfx, st) if t is not None]
    return (out, *extra) if extra else out


# ---- the people mesh overlay (pr_render_people): everybody of a frame on one canvas, depth-tested against each other ----------
Z_STEP_MAX = 1 << 24        # PR_RENDER_Z_STEP_MAX, 4096 m in depth steps
Z_FIX = 4096.0              # depth steps per metre


def people_z_step(cam, bboxes, scale, H, W):
    """The one host rule that orders the people of a frame in depth from their weak-perspective cameras: cam [N,3] (s, tx, ty),
    bboxes [N,4] (cx, cy, w, h), scale = cfg.DATASET.bbox_scale, the frame's H and W -> z_step int32[N] for overlay_people.

    A metre of the body spans ppm = s scale (w + h) / 4 pixels (the projection's s w scale / 2 and s h scale / 2, averaged),
    evaluated in float64.  Under a pinhole camera of focal length hypot(H, W) px that is a depth of d = hypot(H, W) / ppm
    metres; z_step = min(rint(4096 d), 2^24), and 0 where s or ppm is not finite or not positive.  The order of the people
    depends on ppm alone: who is drawn larger is nearer.  The focal length -- an ASSUMPTION, a 53 degree diagonal field of
    view -- only sets how far apart they stand compared with a body's own +-0.5 m of depth.  The rule has not been checked
    against true occlusion on real video."""
    c = np.asarray(cam, np.float64).reshape(-1, 3)
    b = np.asarray(bboxes, np.float64).reshape(-1, 4)
    if c.shape[0] != b.shape[0]:
        raise ValueError(f"{c.shape[0]} cameras for {b.shape[0]} boxes")
    s = c[:, 0]
    with np.errstate(all="ignore"):
        ppm = s * float(scale) * (b[:, 2] + b[:, 3]) / 4.0
        ok = np.isfinite(s) & (s > 0) & np.isfinite(ppm) & (ppm > 0)
        d = float(np.hypot(float(H), float(W))) / np.where(ok, ppm, 1.0)
        z = np.minimum(np.rint(Z_FIX * d), float(Z_STEP_MAX))
    return np.where(ok, z, 0.0).astype(np.int32)


def _host_ints(x, n, what):
    a = x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
    if a.shape != (n,) or a.dtype.kind not in "iu":
        raise ValueError(f"{what} must be int[{n}], got {a.dtype}{list(a.shape)}")
    return a.astype(np.int32)


def overlay_people(frames, verts, faces, cam, bboxes, canvas, src_idx, z_step=None, scale=1.2, face_part=None, part_rgb=None,
                   alpha=0.6, bgr=False, out=None, return_face_id=False, return_vert_fx=False, return_status=False,
                   return_canvas_status=False):
    """Draw N meshes on M canvases on the GPU, the meshes of a canvas depth-tested against each other (pr_render_people; the
    contract is section r4 of include/poserisk_hip.h).

    As `overlay`, with canvas int[N] (the canvas of each mesh), src_idx int[M] (the source frame of each canvas) and z_step
    int[N] or None (all zero; people_z_step makes it from the cameras) in place of frame_idx.  Returns out u8[M,H,W,3],
    followed by face_id int32[M,H,W] (n F + f), vert_fx int32[N,V,4], status int32[N] and canvas_status int32[M] as asked
    for.  Shapes and face indices are checked here, once, on the host, before anything goes to the device; indices in
    canvas, src_idx and z_step outside their ranges are the kernel's to flag (status bits 3, 4, and canvas_status)."""
    if not isinstance(frames, torch.Tensor) or frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[3] != 3:
        raise ValueError("frames must be a uint8 tensor [n_frames,H,W,3]")
    n_frames, H, W, _ = frames.shape
    vshape = tuple(verts.shape) if hasattr(verts, "shape") else np.shape(verts)
    if len(vshape) != 3 or vshape[2] != 3:
        raise ValueError(f"verts must have shape (N, V, 3), got {tuple(vshape)}")
    N, V = int(vshape[0]), int(vshape[1])
    faces_host = _host_faces(faces, V)
    F = faces_host.shape[0]
    cv = _host_ints(canvas, N, "canvas")
    M = int(np.shape(src_idx)[0]) if np.ndim(src_idx) == 1 else -1
    if M < 0:
        raise ValueError(f"src_idx must be int[M], got shape {tuple(np.shape(src_idx))}")
    si = _host_ints(src_idx, M, "src_idx")
    zs = None if z_step is None else _host_ints(z_step, N, "z_step")
    if N * F >= 1 << 31:
        raise ValueError(f"N F = {N * F} does not fit the key's low half (2^31)")
    if frames.device.type != "cuda":
        raise _lib.PoseRiskHipError("overlay_people: frames must be a CUDA tensor (no CPU fallback)")
    dev = frames.device
    frames = frames.contiguous()
    v = _dev_tensor(verts, torch.float32, dev, (N, V, 3), "verts")
    f, c, bb, fp, rgb = _mesh_tensors(faces, faces_host, cam, bboxes, face_part, part_rgb, N, dev, min_parts=1)
    cv, si = torch.from_numpy(cv).to(dev), torch.from_numpy(si).to(dev)
    zs = None if zs is None else torch.from_numpy(zs).to(dev)
    out, fid, vfx, st = _outputs(out, M, "M", N, V, H, W, dev, return_face_id, return_vert_fx, return_status)
    cst = torch.empty((M,), dtype=torch.int32, device=dev) if return_canvas_status else None
    lib = _lib.load()
    nbytes = lib.pr_render_people_workspace_bytes(N, M, V, F, H, W)
    ws = torch.empty((max(int(nbytes), 1),), dtype=torch.uint8, device=dev)
    args = _lib.RenderPeopleArgs(v.data_ptr(), f.data_ptr(), c.data_ptr(), bb.data_ptr(), frames.data_ptr(), cv.data_ptr(),
                                 si.data_ptr(), _ptr(zs), fp.data_ptr(), rgb.data_ptr(), out.data_ptr(), _ptr(fid), _ptr(vfx),
                                 _ptr(st), _ptr(cst), N, M, V, F, rgb.shape[1], n_frames, H, W, int(bool(bgr)), float(scale),
                                 float(alpha))
    _lib.check(lib.pr_render_people(args, ws.data_ptr(), nbytes, torch.cuda.current_stream(dev).cuda_stream),
               "pr_render_people")
    extra = [t for t in (fid, vfx, st, cst) if t is not None]
    return (out, *extra) if extra else out
