"""CPU-only: the mesh overlay's raster contract as restated in tests/raster_ref.py (watertight coverage, depth order and
ties, the projection against the crop's affine), the part / colour tables of poserisk_release_amd.render, and the argument
checks of pr_render_overlay (they return before any device work)."""
import numpy as np
import pytest

import raster_ref as rr
from oracle import crop_ref
from poserisk_release_amd import _lib, render, synth


def _vfx(xy16, z=0.5):
    """Fixed-point vertices straight from sub-pixel coordinates (16ths of a pixel)."""
    xy16 = np.asarray(xy16, np.int64)
    out = np.zeros((len(xy16), 4), np.int32)
    out[:, :2] = xy16
    out[:, 2] = int(round(4096 * z)) + (1 << 20)
    out[:, 3] = 1
    return out


def _split_quad_grid(nx, ny, x0, y0, step, rng, jitter):
    """(nx+1) x (ny+1) vertices, interior ones jittered, each quad split along a random diagonal with a random winding."""
    gx, gy = np.meshgrid(np.arange(nx + 1), np.arange(ny + 1))
    xy = np.stack([x0 + gx * step, y0 + gy * step], -1).reshape(-1, 2).astype(np.int64)
    interior = ((gx > 0) & (gx < nx) & (gy > 0) & (gy < ny)).reshape(-1)
    xy[interior] += rng.integers(-jitter, jitter + 1, (int(interior.sum()), 2))
    vid = lambda i, j: j * (nx + 1) + i
    faces = []
    for j in range(ny):
        for i in range(nx):
            a, b, c, d = vid(i, j), vid(i + 1, j), vid(i, j + 1), vid(i + 1, j + 1)
            tris = [(a, b, d), (a, d, c)] if rng.random() < 0.5 else [(a, b, c), (b, d, c)]
            faces += [t if rng.random() < 0.5 else (t[0], t[2], t[1]) for t in tris]
    return xy, np.array(faces, np.int32)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_split_quad_grid_is_watertight(seed):
    rng = np.random.default_rng(seed)
    H, W = 40, 48
    # outer boundary on sample rows / columns (multiples of 16) so that "interior" is exact; vertices on and off samples
    xy, faces = _split_quad_grid(9, 7, 16 * 3, 16 * 2, 64 + 16 * seed // 2, rng, jitter=20)
    count = rr.coverage_count(_vfx(xy), faces, H, W)
    x_lo, y_lo = xy[:, 0].min() // 16, xy[:, 1].min() // 16
    x_hi, y_hi = xy[:, 0].max() // 16, xy[:, 1].max() // 16
    inner = count[y_lo + 1:y_hi, x_lo + 1:x_hi]
    assert inner.size > 500 and inner.min() == 1 and inner.max() == 1, np.unique(inner, return_counts=True)
    # on the whole frame nothing is covered twice either (shared boundary samples go to one face)
    assert count.max() == 1


@pytest.mark.parametrize("n_ring", [5, 12, 31])
def test_triangle_fan_is_watertight(n_ring):
    rng = np.random.default_rng(n_ring)
    H, W = 40, 40
    cx, cy = 16 * 20, 16 * 19                               # the shared vertex sits exactly on a sample
    ang = np.sort(rng.uniform(0, 2 * np.pi, n_ring))
    r = 16 * 14 / np.maximum(np.abs(np.cos(ang)), np.abs(np.sin(ang)))   # ring on the square of half-side 14 px
    ring = np.stack([cx + np.rint(r * np.cos(ang)), cy + np.rint(r * np.sin(ang))], -1)
    corners = np.array([[cx + 224, cy + 224], [cx - 224, cy + 224], [cx - 224, cy - 224], [cx + 224, cy - 224]])
    pts = np.concatenate([ring, corners])
    a = np.arctan2(pts[:, 1] - cy, pts[:, 0] - cx) % (2 * np.pi)
    pts = pts[np.argsort(a)]
    xy = np.concatenate([[[cx, cy]], pts]).astype(np.int64)
    m = len(pts)
    faces = np.array([(0, 1 + k, 1 + (k + 1) % m) for k in range(m)], np.int32)
    count = rr.coverage_count(_vfx(xy), faces, H, W)
    inner = count[cy // 16 - 13:cy // 16 + 14, cx // 16 - 13:cx // 16 + 14]
    assert inner.min() == 1 and inner.max() == 1
    assert count.max() == 1


def test_nearer_face_wins_and_depth_ties_go_to_lower_index():
    H, W = 20, 20
    tri = [[16, 16], [16 * 18, 16 * 2], [16 * 3, 16 * 17]]
    near, far = _vfx(tri, z=1.0), _vfx(tri, z=2.0)
    v = np.concatenate([far, near])
    faces = np.array([[0, 1, 2], [3, 4, 5]], np.int32)       # face 0 far, face 1 near
    fid = rr.face_id(rr.raster_keys(v, faces, H, W))
    assert (fid == 1).sum() > 50 and not (fid == 0).any()
    fid = rr.face_id(rr.raster_keys(v, faces[::-1].copy(), H, W))   # order of the faces does not matter, the depth does
    assert (fid == 0).sum() > 50 and not (fid == 1).any()
    same = np.concatenate([near, near])
    for order in ([[0, 1, 2], [3, 5, 4]], [[3, 4, 5], [0, 2, 1]]):   # duplicated coplanar faces, either winding
        fid = rr.face_id(rr.raster_keys(same, np.array(order, np.int32), H, W))
        assert (fid == 0).sum() > 50 and not (fid == 1).any()
    # depth is interpolated: a tilted face beats a flat one where it is nearer only
    tilt = near.copy()
    tilt[1, 2] -= 8192                                      # vertex 1 two metres nearer
    fid = rr.face_id(rr.raster_keys(np.concatenate([tilt, _vfx(tri, z=0.9)]), faces, H, W))
    assert (fid == 0).any() and (fid == 1).any()


def test_zero_area_and_invalid_faces_draw_nothing():
    v = _vfx([[16, 16], [160, 160], [320, 320], [16, 300]])
    keys = rr.raster_keys(v, np.array([[0, 1, 2]], np.int32), 30, 30)   # collinear
    assert (keys == rr.EMPTY).all()
    v[3, 3] = 0
    keys = rr.raster_keys(v, np.array([[0, 2, 3]], np.int32), 30, 30)
    assert (keys == rr.EMPTY).all()


def test_projection_inverts_the_crop_affine():
    rng = np.random.default_rng(5)
    N, V = 6, 50
    verts = rng.normal(0, 0.4, (N, V, 3))
    cam = np.stack([rng.uniform(0.6, 1.2, N), rng.normal(0, 0.1, N), rng.normal(0, 0.1, N)], 1)
    bboxes = np.stack([rng.uniform(200, 600, N), rng.uniform(150, 300, N), rng.uniform(80, 300, N),
                       rng.uniform(80, 300, N)], 1).astype(np.float32)
    x, y, z = rr.project(verts, cam, bboxes, 1.2, 450, 800)
    for n in range(N):
        M = crop_ref.affine_from_bbox(bboxes[n], 1.2)
        u = M[0, 0] * x[n] + M[0, 1] * y[n] + M[0, 2]
        w = M[1, 0] * x[n] + M[1, 1] * y[n] + M[1, 2]
        np.testing.assert_allclose(u, 112 * (1 + cam[n, 0] * (verts[n, :, 0] + cam[n, 1])), atol=2e-3)
        np.testing.assert_allclose(w, 112 * (1 + cam[n, 0] * (verts[n, :, 1] + cam[n, 2])), atol=2e-3)
    np.testing.assert_array_equal(z, verts[..., 2])


def test_vert_fx_rounding_and_validity():
    H, W = 10, 20
    verts = np.array([[[0.0, 0.0, 0.0], [1 / 32, 3 / 32, 1 / 8192], [np.nan, 0, 0], [0, 0, 256.0], [4115.0, 0, 0]]])   # x = 4120 >= W - 1 + 4096
    cam = np.array([[1.0, 0.0, 0.0]])
    bb = np.array([[5.0, 5.0, 2.0, 2.0]])          # x = 5 + X, y = 5 + Y at scale 1
    fx = rr.vert_fx(verts, cam, bb, 1.0, H, W)[0]
    np.testing.assert_array_equal(fx[0], [80, 80, 1 << 20, 1])
    np.testing.assert_array_equal(fx[1], [80, 82, (1 << 20) + 0, 1])   # 80.5 -> 80, 81.5 -> 82 (half to even), 0.5 -> 0
    assert not fx[2:, 3].any() and not fx[2:, :3].any()


def test_face_parts_table():
    faces = np.array([[0, 1, 2]], np.int32)
    for j in range(24):
        w = np.zeros((3, 24), np.float32)
        w[:, j] = 1
        got = int(render.face_parts(w, faces, "REBA")[0])
        assert render.PARTS[got] == {**{k: "trunk" for k in (0, 3, 6, 9, 13, 14)}, 12: "neck", 15: "neck",
                                     **{k: "leg" for k in (1, 2, 4, 5, 7, 8, 10, 11)},
                                     16: "upper_arm_l", 17: "upper_arm_r", 18: "lower_arm_l", 19: "lower_arm_r",
                                     20: "wrist_l", 22: "wrist_l", 21: "wrist_r", 23: "wrist_r"}[j], j
    # the face's three vertices' weights are summed before the argmax
    w = np.zeros((3, 24), np.float32)
    w[0, 16] = 0.9
    w[1, 18], w[2, 18] = 0.5, 0.5
    assert render.PARTS[render.face_parts(w, faces, "RULA")[0]] == "lower_arm_l"
    assert render.face_parts(w, faces, None).tolist() == [0]
    with pytest.raises(ValueError):
        render.face_parts(w, faces, "OWAS")


def test_part_colours_table():
    g, y, o, r = (render.LEVEL_RGB[k].tolist() for k in range(4))
    reba = np.array([[11, 1, 2, 3, 4, 5, 0, 2, 9, 1]], np.int32)   # score, trunk, neck, leg, ua L,R, la L,R, wr L,R
    got = render.part_colours(reba, "REBA")[0].tolist()
    assert got == [g, y, o, r, r, g, y, r, g]
    rula = np.array([[7, 1, 2, 3, 4, 1, 2, 3, 3, 4, 2, 1]], np.int32)   # score, ua L,R, la L,R, wr L,R, twist L,R, neck, trunk, leg
    got = render.part_colours(rula, "RULA")[0].tolist()
    assert got == [y, r, g, g, y, o, r, g, y]                         # trunk, neck, leg, ua L,R, la L,R, wr L,R
    assert render.part_colours(rula, None).shape == (1, 1, 3)
    with pytest.raises(ValueError):
        render.part_colours(reba, "RULA")


def test_genus0_mesh_is_closed_with_smpl_counts():
    f = synth.genus0_mesh(6890)[1]
    assert f.shape == (13776, 3) and f.min() == 0 and f.max() == 6889
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    s = set(map(tuple, e.tolist()))
    assert len(s) == len(e) and all((b, a) in s for a, b in s)


def _args(**kw):
    fake = 256                                   # never dereferenced: every check below fails before device work
    a = dict(verts=fake, faces=fake, cam=fake, bboxes=fake, frames=fake, frame_idx=None, face_part=fake, part_rgb=fake,
             out=fake, face_id=None, vert_fx=None, status=None, N=2, V=10, F=4, P=1, n_frames=2, H=45, W=80, bgr=0,
             scale=1.2, alpha=0.5)
    a.update(kw)
    return _lib.RenderArgs(**a)


def test_render_entry_argument_checks():
    lib = _lib.load()
    assert lib.pr_render_workspace_bytes(0, 10, 4, 45, 80) == 0
    ws = lib.pr_render_workspace_bytes(2, 10, 4, 45, 80)
    assert ws >= 2 * 45 * 80 * 8 + 2 * 10 * 16 + 2 * 4 * 4 * 2
    assert lib.pr_render_overlay(_args(N=0, verts=None, out=None), None, 0, None) == 0          # N = 0: nothing to do
    assert lib.pr_render_overlay(None, 256, ws, None) == -1
    for name in ("verts", "faces", "cam", "bboxes", "frames", "face_part", "part_rgb", "out"):
        assert lib.pr_render_overlay(_args(**{name: None}), 256, ws, None) == -1, name
        assert "null" in lib.pr_last_error().decode()
    assert lib.pr_render_overlay(_args(), None, ws, None) == -1
    assert lib.pr_render_overlay(_args(H=4097), 256, 1 << 40, None) == -1
    assert "4096" in lib.pr_last_error().decode()
    assert lib.pr_render_overlay(_args(W=5000), 256, 1 << 40, None) == -1
    assert lib.pr_render_overlay(_args(N=-1), 256, ws, None) == -1
    assert lib.pr_render_overlay(_args(alpha=1.5), 256, ws, None) == -1
    assert lib.pr_render_overlay(_args(N=3), 256, 1 << 40, None) == -1          # 3 crops, 2 frames, no frame index
    assert lib.pr_render_overlay(_args(), 256, ws - 1, None) == -1
    assert "workspace" in lib.pr_last_error().decode()


def test_overlay_wrapper_refuses_cpu_frames_and_bad_faces():
    import torch
    with pytest.raises(_lib.PoseRiskHipError):
        render.overlay(torch.zeros((1, 4, 4, 3), dtype=torch.uint8), np.zeros((1, 3, 3)), [[0, 1, 2]], np.ones((1, 3)),
                       np.ones((1, 4)))
