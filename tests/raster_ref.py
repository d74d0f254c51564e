"""numpy restatement of the mesh overlay's raster contract (include/poserisk_hip.h, pr_render_overlay): fixed point and
coverage in int64, keys as uint64, shading and compositing in float64.  Test infrastructure: the kernels in
poserisk_release_amd/csrc/render.hip are compared with it, face_id bit for bit when it is fed the GPU's own vert_fx."""
import numpy as np

FIX, ZFIX, ZBIAS, GUARD, ZMAX = 16.0, 4096.0, 1 << 20, 4096.0, 256.0
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)


def project(verts, cam, bboxes, scale, H, W):
    """verts [N,V,3], cam [N,3], bboxes [N,4] -> (x, y, Z) float64 [N,V] each."""
    v = np.asarray(verts, np.float64)
    c = np.asarray(cam, np.float64)[:, None, :]
    b = np.asarray(bboxes, np.float64)[:, None, :]
    s = float(np.float32(scale))
    x = b[..., 0] + c[..., 0] * (v[..., 0] + c[..., 1]) * b[..., 2] * s * 0.5
    y = b[..., 1] + c[..., 0] * (v[..., 1] + c[..., 2]) * b[..., 3] * s * 0.5
    return x, y, v[..., 2]


def vert_fx(verts, cam, bboxes, scale, H, W):
    """-> int32 [N,V,4] (xf, yf, zf, valid), zeros where invalid."""
    x, y, z = project(verts, cam, bboxes, scale, H, W)
    with np.errstate(invalid="ignore"):
        valid = (np.isfinite(x) & np.isfinite(y) & np.isfinite(z) & (x > -GUARD) & (x < W - 1 + GUARD) & (y > -GUARD)
                 & (y < H - 1 + GUARD) & (np.abs(z) < ZMAX))
    out = np.zeros(x.shape + (4,), np.int32)
    out[..., 0] = np.where(valid, np.rint(FIX * np.where(valid, x, 0)), 0)
    out[..., 1] = np.where(valid, np.rint(FIX * np.where(valid, y, 0)), 0)
    out[..., 2] = np.where(valid, np.rint(ZFIX * np.where(valid, z, 0)) + ZBIAS, 0)
    out[..., 3] = valid
    return out


def _orient(ax, ay, bx, by, cx, cy):
    return (bx - ax) * (cy - ay) - (by - ay) * (cx - ax)


def _owns(dx, dy):
    return (dy > 0) | ((dy == 0) & (dx < 0))


def raster_keys(vfx, faces, H, W, max_pairs=1 << 22):
    """One crop: vfx int32 [V,4], faces int [F,3] -> keys uint64 [H,W] (~0 where empty)."""
    vfx = np.asarray(vfx, np.int64)
    faces = np.asarray(faces, np.int64)
    V = vfx.shape[0]
    keys = np.full(H * W, EMPTY, np.uint64)
    ok_idx = np.all((faces >= 0) & (faces < V), axis=1)
    fidx = np.nonzero(ok_idx)[0]
    f = faces[fidx]
    a, b, c = vfx[f[:, 0]], vfx[f[:, 1]], vfx[f[:, 2]]
    valid = (a[:, 3] != 0) & (b[:, 3] != 0) & (c[:, 3] != 0)
    A = _orient(a[:, 0], a[:, 1], b[:, 0], b[:, 1], c[:, 0], c[:, 1])
    keep = valid & (A != 0)
    fidx, a, b, c, A = fidx[keep], a[keep], b[keep], c[keep], A[keep]
    neg = A < 0
    b, c = np.where(neg[:, None], c, b), np.where(neg[:, None], b, c)
    A = np.abs(A)
    xs = np.stack([a[:, 0], b[:, 0], c[:, 0]], 1)
    ys = np.stack([a[:, 1], b[:, 1], c[:, 1]], 1)
    x0 = np.maximum((xs.min(1) + 15) >> 4, 0)
    x1 = np.minimum(xs.max(1) >> 4, W - 1)
    y0 = np.maximum((ys.min(1) + 15) >> 4, 0)
    y1 = np.minimum(ys.max(1) >> 4, H - 1)
    keep = (x0 <= x1) & (y0 <= y1)
    fidx, a, b, c, A, x0, x1, y0, y1 = (t[keep] for t in (fidx, a, b, c, A, x0, x1, y0, y1))
    bw, bh = x1 - x0 + 1, y1 - y0 + 1
    cnt = bw * bh
    start = 0
    while start < len(fidx):
        # a chunk of faces whose boxes hold at most max_pairs samples (at least one face)
        csum = np.cumsum(cnt[start:])
        stop = start + max(1, int(np.searchsorted(csum, max_pairs, side="right")))
        sl = slice(start, stop)
        n = cnt[sl]
        rep = np.repeat(np.arange(stop - start), n)
        local = np.arange(int(n.sum()), dtype=np.int64) - np.repeat(np.cumsum(n) - n, n)
        bw_r = bw[sl][rep]
        py = 16 * (y0[sl][rep] + local // bw_r)
        px = 16 * (x0[sl][rep] + local % bw_r)
        aa, bb, cc = a[sl][rep], b[sl][rep], c[sl][rep]
        w0 = _orient(bb[:, 0], bb[:, 1], cc[:, 0], cc[:, 1], px, py)
        w1 = _orient(cc[:, 0], cc[:, 1], aa[:, 0], aa[:, 1], px, py)
        w2 = _orient(aa[:, 0], aa[:, 1], bb[:, 0], bb[:, 1], px, py)
        in0 = (w0 > 0) | ((w0 == 0) & _owns(cc[:, 0] - bb[:, 0], cc[:, 1] - bb[:, 1]))
        in1 = (w1 > 0) | ((w1 == 0) & _owns(aa[:, 0] - cc[:, 0], aa[:, 1] - cc[:, 1]))
        in2 = (w2 > 0) | ((w2 == 0) & _owns(bb[:, 0] - aa[:, 0], bb[:, 1] - aa[:, 1]))
        cov = in0 & in1 & in2
        depth = (w0 * aa[:, 2] + w1 * bb[:, 2] + w2 * cc[:, 2])[cov] // A[sl][rep][cov]
        key = (depth.astype(np.uint64) << np.uint64(32)) | fidx[sl][rep][cov].astype(np.uint64)
        np.minimum.at(keys, (py[cov] // 16) * W + px[cov] // 16, key)
        start = stop
    return keys.reshape(H, W)


def face_id(keys):
    return np.where(keys == EMPTY, -1, (keys & np.uint64(0xFFFFFFFF)).astype(np.int64)).astype(np.int32)


def coverage_count(vfx, faces, H, W):
    """How many faces cover each sample (the watertightness check): int [H,W]."""
    count = np.zeros((H, W), np.int64)
    for f in range(len(faces)):
        k = raster_keys(vfx, np.asarray(faces)[f:f + 1], H, W)
        count += k != EMPTY
    return count


def face_colours(verts, faces, face_part, part_rgb, bgr=False):
    """One crop: float64 [F,3] colour per face in the frame's channel order."""
    v = np.asarray(verts, np.float64)
    f = np.asarray(faces, np.int64)
    n = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    ln = np.linalg.norm(n, axis=1)
    nz = np.where(ln > 0, np.abs(n[:, 2]) / np.where(ln > 0, ln, 1), 0.0)
    inten = 0.35 + 0.65 * nz
    rgb = np.asarray(part_rgb, np.float64)[np.clip(np.asarray(face_part), 0, len(part_rgb) - 1)]
    if bgr:
        rgb = rgb[:, ::-1]
    return rgb * inten[:, None]


def composite(frame, fid, colours, alpha):
    """frame u8 [H,W,3], face_id [H,W], colours float64 [F,3] -> out u8 [H,W,3]."""
    out = frame.copy()
    m = fid >= 0
    blend = (1.0 - alpha) * frame[m].astype(np.float64) + alpha * colours[fid[m]]
    out[m] = np.clip(np.rint(blend), 0, 255).astype(np.uint8)
    return out
