"""numpy restatement of the people mesh overlay's contract (include/poserisk_hip.h section r4, pr_render_people) on top of
tests/raster_ref.py: every mesh is rasterised on its own with zf shifted by its z_step, the low half of its keys is rewritten
to n F + f, and a canvas takes the smallest key of its meshes per pixel.  Test infrastructure: face_id of the kernels in
poserisk_release_amd/csrc/render.hip is compared with it bit for bit when it is fed the GPU's own vert_fx."""
import numpy as np

import raster_ref as rr

Z_STEP_MAX = 1 << 24
LOW = np.uint64(0xFFFFFFFF)


def mesh_status(canvas, src_idx, z_step, n_frames):
    """Bits 0, 3 and 4 of status int32[N], and canvas_status int32[M]."""
    canvas, src_idx = np.asarray(canvas, np.int64), np.asarray(src_idx, np.int64)
    z = np.zeros(len(canvas), np.int64) if z_step is None else np.asarray(z_step, np.int64)
    bad_src = (src_idx < 0) | (src_idx >= n_frames)
    st = np.where((canvas < 0) | (canvas >= len(src_idx)), 8, 0) | np.where((z < 0) | (z > Z_STEP_MAX), 16, 0)
    on_bad = bad_src[np.clip(canvas, 0, max(len(src_idx) - 1, 0))] if len(src_idx) else np.zeros(len(canvas), bool)
    st = np.where((st == 0) & on_bad, 1, st)
    return st.astype(np.int32), bad_src.astype(np.int32)


def vert_fx(verts, cam, bboxes, scale, H, W, z_step=None, dead=None):
    """raster_ref.vert_fx with zf shifted by z_step AFTER the rounding (valid vertices only); rows of `dead` meshes (status
    bit 3 or 4) are all zero."""
    fx = rr.vert_fx(verts, cam, bboxes, scale, H, W)
    if z_step is not None:
        fx[..., 2] += np.where(fx[..., 3] != 0, np.asarray(z_step, np.int64)[:, None], 0).astype(np.int32)
    if dead is not None:
        fx[np.asarray(dead, bool)] = 0
    return fx


def canvas_keys(vfx, faces, canvas, src_idx, z_step, n_frames, H, W):
    """vfx int32[N,V,4] (zf already shifted, as pr_render_people's vert_fx output is), faces int[F,3] -> keys uint64[M,H,W]
    with the low half n F + f (~0 where empty)."""
    vfx, faces = np.asarray(vfx), np.asarray(faces)
    F, M = len(faces), len(src_idx)
    st, _ = mesh_status(canvas, src_idx, z_step, n_frames)
    keys = np.full((M, H, W), rr.EMPTY, np.uint64)
    for n in range(len(vfx)):
        if st[n]:
            continue
        k = rr.raster_keys(vfx[n], faces, H, W)
        hit = k != rr.EMPTY
        k = np.where(hit, (k & ~LOW) | ((k & LOW) + np.uint64(n * F)), k)
        m = int(canvas[n])
        keys[m] = np.minimum(keys[m], k)
    return keys


def render(frames, verts, faces, canvas, src_idx, keys, face_part, part_rgb, alpha, bgr=False):
    """keys from canvas_keys -> (out u8[M,H,W,3] with the float64 blend, face_id int32[M,H,W]).  A canvas with a bad src_idx is
    zero-filled and its face_id -1."""
    frames = np.asarray(frames)
    N, F, M = len(verts), len(faces), len(src_idx)
    colours = (np.concatenate([rr.face_colours(verts[n], faces, face_part, part_rgb[n], bgr) for n in range(N)]) if N
               else np.zeros((0, 3)))
    fid = rr.face_id(keys)
    out = np.zeros((M,) + frames.shape[1:], np.uint8)
    for m in range(M):
        if not 0 <= int(src_idx[m]) < len(frames):
            fid[m] = -1
            continue
        out[m] = rr.composite(frames[int(src_idx[m])], fid[m], colours, alpha)
    return out, fid
