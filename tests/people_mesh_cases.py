"""Scene builders for the people mesh overlay's tests (pr_render_people; tests/test_people_mesh_gpu.py and
tests/test_people_mesh_cpu.py).  Every builder returns a dict with verts f32[N,V,3], faces int32[F,3], cam f32[N,3] and bboxes
f32[N,4]; the soups and grids are in pixel coordinates under the identity projection (IDENT_CAM, ident_bbox), depth in metres."""
import numpy as np

from poserisk_release_amd import synth

SCALE = 1.2
SIZES = ((37, 53), (96, 128))                                   # (H, W)
IDENT_CAM = (1.0, 0.0, 0.0)


def ident_bbox(scale=SCALE):
    """A box for which the projection is the identity: x = X, y = Y (pixels)."""
    return (0.0, 0.0, 2.0 / scale, 2.0 / scale)


def _ident(verts, faces):
    N = len(verts)
    return dict(verts=np.asarray(verts, np.float32), faces=np.asarray(faces, np.int32),
                cam=np.tile(np.array(IDENT_CAM, np.float32), (N, 1)), bboxes=np.tile(np.array(ident_bbox(), np.float32), (N, 1)))


def soup(N, H, W, seed, n_tri=160):
    """Per mesh n_tri independent triangles: two frame-spanning faces (the big-face queue), slivers, zero-area faces, faces
    partly and wholly off the frame, small and medium ones, and duplicated coplanar faces of either winding."""
    faces = np.arange(3 * n_tri).reshape(-1, 3)
    faces = np.concatenate([faces, faces[5:45:4, ::-1], faces[7:47:8]])
    verts = []
    for n in range(N):
        rng = np.random.default_rng(seed * 100 + n)
        tris = [[[-0.3 * W, -0.2 * H], [1.4 * W, -0.1 * H], [0.4 * W, 1.5 * H]], [[1.2 * W, 1.3 * H], [-0.5 * W, 0.9 * H], [0.8 * W, -0.6 * H]]]
        for _ in range(12):
            p, d = rng.uniform([0, 0], [W, H]), rng.normal(0, 1, 2)
            tris.append([p, p + 30 * d, p + 30 * d + rng.normal(0, 0.05, 2)])
        for _ in range(6):
            p, d = rng.uniform([0, 0], [W, H]), rng.normal(0, 5, 2)
            tris.append([p, p + d, p + 2 * d] if rng.random() < 0.5 else [p, p, p + d])
        for _ in range(10):
            p = rng.uniform([-40, -40], [W + 40, H + 40])
            tris.append([p, p + rng.normal(0, 20, 2), p + rng.normal(0, 20, 2)])
        tris.append([[W + 100.0, 5.0], [W + 120.0, 10.0], [W + 105.0, 25.0]])
        while len(tris) < n_tri:
            p, s = rng.uniform([0, 0], [W, H]), rng.choice([1.5, 5.0, 14.0])
            tris.append([p, p + rng.normal(0, s, 2), p + rng.normal(0, s, 2)])
        xy = np.array(tris, np.float64).reshape(-1, 2)
        z = np.repeat(rng.uniform(1, 10, n_tri), 3) + rng.normal(0, 0.3, 3 * n_tri)
        verts.append(np.concatenate([xy, z[:, None]], 1))
    return _ident(verts, faces)


def grid(N, H, W, seed, tilt=None, nx=13, ny=9):
    """Per mesh a jittered split-quad grid over most of the frame.  Depth: a gentle wave around 3 m, or, with tilt = [(z0, dz/dx
    m per px)] per mesh, a plane -- two opposite tilts cross inside the frame."""
    verts, faces = [], None
    for n in range(N):
        rng = np.random.default_rng(seed * 100 + n)
        gx, gy = np.meshgrid(np.linspace(-0.05 * W, 0.95 * W, nx + 1), np.linspace(0.08 * H, 1.05 * H, ny + 1))
        xy = np.stack([gx, gy], -1).reshape(-1, 2) + rng.normal(0, 0.15 * W / nx, ((nx + 1) * (ny + 1), 2))
        if tilt is None:
            z = 3 + 0.5 * np.sin(xy[:, :1] / 17) + 0.2 * np.cos(xy[:, 1:] / 11)
        else:
            z = tilt[n][0] + tilt[n][1] * xy[:, :1]
        verts.append(np.concatenate([xy, z], 1))
        if faces is None:
            vid = lambda i, j: j * (nx + 1) + i
            faces = []
            for j in range(ny):
                for i in range(nx):
                    a, b, c, d = vid(i, j), vid(i + 1, j), vid(i, j + 1), vid(i + 1, j + 1)
                    faces += [(a, b, d), (a, d, c)] if rng.random() < 0.5 else [(a, b, c), (c, b, d)]
    return _ident(verts, faces)


def spanning(N, H, W, seed):
    """Per mesh four faces that each cover much of the frame, tilted in depth so that faces of different meshes cross."""
    verts = []
    for n in range(N):
        rng = np.random.default_rng(seed * 100 + n)
        xy = rng.uniform([-0.4 * W, -0.4 * H], [1.4 * W, 1.4 * H], (12, 2))
        verts.append(np.concatenate([xy, rng.uniform(2, 6, (12, 1))], 1))
    return _ident(verts, np.arange(12).reshape(4, 3))


def bodies(N, H, W, seed, V=6890):
    """N person-sized closed meshes (synth.closed_body) turned about the vertical axis, with weak-perspective cameras and
    square tracker-like boxes of different sizes scattered over the frame, so that they overlap."""
    rng = np.random.default_rng(seed)
    v, faces = synth.closed_body(V)
    verts, cams, boxes = [], [], []
    for n in range(N):
        a = rng.uniform(-0.6, 0.6)
        R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
        verts.append(v @ R.T)
        cams.append([rng.uniform(0.8, 1.0), rng.normal(0, 0.05), rng.normal(0, 0.05)])
        h = rng.uniform(0.4, 0.9) * H
        boxes.append([rng.uniform(0.25, 0.75) * W, rng.uniform(0.4, 0.6) * H, h, h])
    return dict(verts=np.array(verts, np.float32), faces=faces, cam=np.array(cams, np.float32), bboxes=np.array(boxes, np.float32))


def frames(n, H, W, seed=3):
    return np.random.default_rng(seed).integers(0, 256, (n, H, W, 3), dtype=np.uint8)


def part_table(N, P, seed=4):
    return np.random.default_rng(seed).integers(0, 256, (N, P, 3), dtype=np.uint8)
