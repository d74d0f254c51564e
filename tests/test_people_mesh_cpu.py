"""CPU: the host half of the people mesh overlay -- render.people_z_step against a float64 restatement, the properties the
contract of pr_render_people rests on as tests/raster_people_ref.py restates it (a uniform integer shift changes nothing, ties
go to the lower mesh), overlay_people's checks before any device call, the ABI surface, and the people_mesh knob."""
import ctypes as C
import math
import os
import re
import types

import numpy as np
import pytest
import torch

import people_mesh_cases as pmc
import raster_people_ref as rpr
import raster_ref as rr
from conftest import REPO
from poserisk_release_amd import _lib, dropin, render


# ---- people_z_step ---------------------------------------------------------------------------------------------------------------
def _z_step_ref(cam, bboxes, scale, H, W):
    out = []
    for (s, _, _), (_, _, w, h) in zip(np.asarray(cam, np.float64).tolist(), np.asarray(bboxes, np.float64).tolist()):
        ppm = s * scale * (w + h) / 4
        if not (math.isfinite(s) and s > 0 and math.isfinite(ppm) and ppm > 0):
            out.append(0)
            continue
        d = math.hypot(H, W) / ppm
        out.append(1 << 24 if 4096 * d >= 1 << 24 else min(int(np.rint(4096 * d)), 1 << 24))
    return out


def test_people_z_step_matches_a_float64_restatement():
    rng = np.random.default_rng(1)
    N = 200
    cam = np.stack([rng.uniform(0.3, 1.5, N), rng.normal(0, 0.1, N), rng.normal(0, 0.1, N)], 1).astype(np.float32)
    bb = np.stack([rng.uniform(0, 800, N), rng.uniform(0, 450, N), rng.uniform(20, 400, N), rng.uniform(20, 400, N)], 1).astype(np.float32)
    for H, W, scale in ((450, 800, 1.2), (96, 128, 1.2), (37, 53, 1.0)):
        z = render.people_z_step(cam, bb, scale, H, W)
        assert z.dtype == np.int32 and z.shape == (N,) and z.tolist() == _z_step_ref(cam, bb, scale, H, W)
        assert z.min() > 0 and z.max() < 1 << 24
        # the order is that of pixels per metre alone: larger on the screen = nearer
        ppm = cam[:, 0].astype(np.float64) * (bb[:, 2].astype(np.float64) + bb[:, 3])
        assert (np.diff(z[np.argsort(-ppm)]) >= 0).all()
    # one worked value: s = 1, a 100 x 100 box at scale 1.2 -> 60 px per metre; hypot(300, 400) = 500 px -> 8.333 m -> 34133
    assert render.people_z_step([[1, 0, 0]], [[0, 0, 100, 100]], 1.2, 300, 400).tolist() == [34133]


def test_people_z_step_edges():
    bb = [[10, 10, 50, 50]]
    for s in (0.0, -0.5, np.nan, np.inf, -np.inf):
        assert render.people_z_step([[s, 0, 0]], bb, 1.2, 96, 128).tolist() == [0], s
    for box in ([0, 0, 0, 0], [0, 0, -30, 10], [0, 0, np.nan, 10], [0, 0, np.inf, 10]):
        assert render.people_z_step([[1.0, 0, 0]], [box], 1.2, 96, 128).tolist() == [0], box
    # the clamp: farther than 4096 m is 2^24, down to the smallest positive size
    assert render.people_z_step([[1e-6, 0, 0], [1e-300, 0, 0], [5e-324, 0, 0]], bb * 3, 1.2, 96, 128).tolist() == [1 << 24] * 3
    d = math.hypot(96, 128)                                                # 160 px
    just = d / 4096 / (1.2 * 25)                                          # ppm = d / 4096: exactly 4096 m
    assert render.people_z_step([[just, 0, 0], [just * 1.001, 0, 0]], bb * 2, 1.2, 96, 128).tolist() == _z_step_ref(
        [[just, 0, 0], [just * 1.001, 0, 0]], bb * 2, 1.2, 96, 128)
    assert render.people_z_step(np.zeros((0, 3)), np.zeros((0, 4)), 1.2, 96, 128).shape == (0,)
    with pytest.raises(ValueError):
        render.people_z_step(np.ones((2, 3)), np.ones((3, 4)), 1.2, 96, 128)
    assert render.Z_STEP_MAX == rpr.Z_STEP_MAX == 1 << 24


# ---- the reference's own properties ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def crowd():
    """16 bodies on one canvas of 96 x 128 and their keys at people_z_step's depths (computed once, left unchanged)."""
    H, W = pmc.SIZES[1]
    sc = pmc.bodies(16, H, W, seed=5)
    z = render.people_z_step(sc["cam"], sc["bboxes"], pmc.SCALE, H, W)
    canvas, src = np.zeros(16, np.int32), np.zeros(1, np.int32)
    keys = rpr.canvas_keys(rpr.vert_fx(sc["verts"], sc["cam"], sc["bboxes"], pmc.SCALE, H, W, z), sc["faces"], canvas, src, z, 1, H, W)
    return sc, z, canvas, src, keys


def test_reference_uniform_shift_changes_no_face_and_one_mesh_ignores_its_step(crowd):
    H, W = pmc.SIZES[1]
    sc, z, canvas, src, keys = crowd
    fid = rr.face_id(keys)
    F = len(sc["faces"])
    assert len(np.unique(fid[fid >= 0] // F)) > 4
    for k in (1, 4095, 1 << 20):
        moved = rpr.canvas_keys(rpr.vert_fx(sc["verts"], sc["cam"], sc["bboxes"], pmc.SCALE, H, W, z + k), sc["faces"], canvas, src, z + k, 1, H, W)
        assert np.array_equal(rr.face_id(moved), fid)
        hit = keys != rr.EMPTY
        assert np.array_equal(moved[hit] >> np.uint64(32), (keys[hit] >> np.uint64(32)) + np.uint64(k))      # the floored depth moves by exactly k
    # a canvas with one mesh: raster_ref's face_id whatever the step
    one = rr.face_id(rr.raster_keys(rr.vert_fx(sc["verts"][3:4], sc["cam"][3:4], sc["bboxes"][3:4], pmc.SCALE, H, W)[0], sc["faces"], H, W))
    for k in (0, 7, 1 << 24):
        vfx = rpr.vert_fx(sc["verts"][3:4], sc["cam"][3:4], sc["bboxes"][3:4], pmc.SCALE, H, W, np.array([k]))
        got = rr.face_id(rpr.canvas_keys(vfx, sc["faces"], canvas[:1], src, np.array([k]), 1, H, W))
        assert np.array_equal(got[0], one) and (one >= 0).any()
    # the bound of the header: zf < 2^25, so the depth numerator stays inside int64 and the depth inside the key's upper half
    top = rpr.vert_fx(sc["verts"], sc["cam"], sc["bboxes"], pmc.SCALE, H, W, np.full(16, 1 << 24))
    assert int(top[..., 2].max()) < 1 << 25 and (2 ** 37) * (2 ** 25) < 2 ** 63


def test_reference_ties_go_to_the_lower_mesh_and_a_step_of_one_decides(crowd):
    H, W = pmc.SIZES[1]
    sc = crowd[0]
    twin = lambda a: np.concatenate([a[:1], a[:1]])
    F = len(sc["faces"])
    canvas, src = np.zeros(2, np.int32), np.zeros(1, np.int32)
    for z, owner in (((0, 0), 0), ((5, 5), 0), ((8, 7), 1), ((7, 8), 0)):
        z = np.array(z)
        vfx = rpr.vert_fx(twin(sc["verts"]), twin(sc["cam"]), twin(sc["bboxes"]), pmc.SCALE, H, W, z)
        fid = rr.face_id(rpr.canvas_keys(vfx, sc["faces"], canvas, src, z, 1, H, W))
        assert (fid >= 0).sum() > 50 and (fid[fid >= 0] // F == owner).all(), (z, owner)


def test_reference_status_and_canvases():
    st, cst = rpr.mesh_status([0, 1, -1, 3, 2, 0, 1], [0, 9, 1], [0, 0, 0, 0, 0, -1, (1 << 24) + 1], n_frames=2)
    assert st.tolist() == [0, 1, 8, 8, 0, 16, 16] and cst.tolist() == [0, 1, 0]
    H, W = pmc.SIZES[0]
    sc = pmc.grid(3, H, W, seed=1)
    canvas, src = np.array([2, 0, 2]), np.array([1, 0, 0])
    vfx = rpr.vert_fx(sc["verts"], sc["cam"], sc["bboxes"], pmc.SCALE, H, W)
    keys = rpr.canvas_keys(vfx, sc["faces"], canvas, src, None, 2, H, W)
    fr = pmc.frames(2, H, W)
    fpart, rgb = np.zeros(len(sc["faces"]), np.int32), pmc.part_table(3, 1)
    out, fid = rpr.render(fr, sc["verts"], sc["faces"], canvas, src, keys, fpart, rgb, 0.6)
    F = len(sc["faces"])
    assert (fid[1] == -1).all() and np.array_equal(out[1], fr[0])          # no mesh: the frame
    assert set(np.unique(fid[0][fid[0] >= 0] // F)) == {1} and set(np.unique(fid[2][fid[2] >= 0] // F)) <= {0, 2}
    # one mesh on a canvas is raster_ref's picture of it
    alone = rr.face_id(rr.raster_keys(vfx[1], sc["faces"], H, W))
    assert np.array_equal(np.where(fid[0] >= 0, fid[0] - F, -1), alone)
    assert np.array_equal(out[0], rr.composite(fr[1], alone, rr.face_colours(sc["verts"][1], sc["faces"], fpart, rgb[1]), 0.6))


# ---- overlay_people: refused on the host, before any device call -----------------------------------------------------------------
def test_overlay_people_refuses_bad_shapes_and_indices_before_any_device_call(monkeypatch):
    monkeypatch.setattr(_lib, "load", lambda: pytest.fail("a device call"))
    fr = torch.zeros((2, 8, 8, 3), dtype=torch.uint8)
    v, f, c, b = np.zeros((3, 4, 3), np.float32), np.array([[0, 1, 2], [1, 2, 3]]), np.ones((3, 3)), np.ones((3, 4))
    cv, si = np.array([0, 1, 1]), np.array([0, 1])
    ok = lambda **kw: render.overlay_people(**{**dict(frames=fr, verts=v, faces=f, cam=c, bboxes=b, canvas=cv, src_idx=si), **kw})
    for kw, word in ((dict(frames=fr.float()), "frames"), (dict(frames=fr[..., :2]), "frames"), (dict(frames=fr.numpy()), "frames"),
                     (dict(verts=v[0]), "verts"), (dict(verts=np.zeros((3, 4, 2))), "verts"),
                     (dict(faces=f[:, :2]), "faces"), (dict(faces=f[:0]), "faces"), (dict(faces=f + 1), r"outside \[0, 4\)"),
                     (dict(faces=f - 1), r"outside \[0, 4\)"), (dict(canvas=cv[:2]), "canvas"), (dict(canvas=cv.astype(np.float32)), "canvas"),
                     (dict(canvas=cv[None]), "canvas"), (dict(src_idx=si[None]), "src_idx"), (dict(src_idx=3), "src_idx"),
                     (dict(z_step=np.zeros(2, np.int32)), "z_step"), (dict(z_step=np.zeros(3)), "z_step")):
        with pytest.raises(ValueError, match=word):
            ok(**kw)
    # everything in order on the host: the next thing it asks for is a GPU
    with pytest.raises(_lib.PoseRiskHipError, match="CUDA tensor"):
        ok()
    with pytest.raises(_lib.PoseRiskHipError, match="CUDA tensor"):
        ok(z_step=np.array([0, 5, 1 << 24]))


# ---- the ABI surface ---------------------------------------------------------------------------------------------------------------
def test_header_binding_and_library_agree():
    hdr = open(os.path.join(REPO, "include", "poserisk_hip.h")).read()
    assert "/* r4 " in hdr and hdr.index("/* r3 ") < hdr.index("/* r4 ") < hdr.index("/* j1 ")
    assert re.search(r"\bint\s+pr_render_people\s*\(\s*const\s+pr_render_people_args\s*\*", hdr)
    assert re.search(r"\bsize_t\s+pr_render_people_workspace_bytes\s*\(\s*int\s+N,\s*int\s+M,\s*int\s+V,\s*int\s+F,\s*int\s+H,\s*int\s+W\)", hdr)
    assert re.search(r"#define\s+PR_RENDER_Z_STEP_MAX\s+\(1\s*<<\s*24\)", hdr)
    assert {"pr_render_people", "pr_render_people_workspace_bytes"} <= set(_lib.SIGNATURES)
    lib = _lib.load()
    assert lib.pr_abi_version() == _lib.ABI_VERSION == 16
    # 15 pointers, 9 ints, 2 floats, padded to 8
    assert C.sizeof(_lib.RenderPeopleArgs) == 15 * 8 + 9 * 4 + 2 * 4 + 4
    fields = re.search(r"typedef struct pr_render_people_args \{(.*?)\} pr_render_people_args;", hdr, re.S).group(1)
    names = re.findall(r"(\w+)\s*(?:;|,)", re.sub(r"/\*.*?\*/", "", fields))
    assert names == [n for n, _ in _lib.RenderPeopleArgs._fields_]
    # the argument checks return before any device work
    assert lib.pr_render_people(None, None, 0, None) == -1 and b"pr_render_people" in lib.pr_last_error()
    assert lib.pr_render_people(C.byref(_lib.RenderPeopleArgs()), None, 0, None) == 0           # M = 0: nothing to do
    fake = 256
    a = dict(verts=fake, faces=fake, cam=fake, bboxes=fake, frames=fake, canvas=fake, src_idx=fake, z_step=None, face_part=fake, part_rgb=fake,
             out=fake, N=2, M=3, V=10, F=4, P=1, n_frames=2, H=45, W=80, bgr=0, scale=1.2, alpha=0.5)
    ws = lib.pr_render_people_workspace_bytes(2, 3, 10, 4, 45, 80)
    assert ws >= 3 * 45 * 80 * 8 + 2 * 10 * 16 + 2 * 4 * 4 * 2
    assert ws - lib.pr_render_people_workspace_bytes(2, 1, 10, 4, 45, 80) >= 2 * 45 * 80 * 8      # the key buffer is sized by M ...
    assert lib.pr_render_workspace_bytes(2, 10, 4, 45, 80) == lib.pr_render_people_workspace_bytes(2, 2, 10, 4, 45, 80)   # ... as r1's is by N
    for over in (dict(M=-1), dict(N=-1), dict(frames=None), dict(out=None), dict(canvas=None), dict(verts=None), dict(H=4097), dict(alpha=2.0),
                 dict(V=2), dict(src_idx=None), dict(scale=0.0), dict(n_frames=0), dict(P=0), dict(N=200000, F=13776), dict(N=1 << 20, V=4096)):
        assert lib.pr_render_people(C.byref(_lib.RenderPeopleArgs(**{**a, **over})), fake, 1 << 40, None) == -1, over
    assert lib.pr_render_people(C.byref(_lib.RenderPeopleArgs(**a)), fake, ws - 1, None) == -1 and b"workspace" in lib.pr_last_error()
    assert lib.pr_render_people(C.byref(_lib.RenderPeopleArgs(**a)), None, ws, None) == -1


# ---- the knob --------------------------------------------------------------------------------------------------------------------
def test_people_mesh_needs_persons_all():
    dropin.install()
    from core import base
    from core.config import cfg
    assert cfg.DATASET.people_mesh is False
    make = lambda **knobs: base.Predictor(types.SimpleNamespace(gpu="0", type="REBA", debug=False, debug_joints="", debug_frame=-1, **knobs),
                                          spin_model=torch.nn.Identity(), smpl_model=object())
    for knobs in (dict(people_mesh=True), dict(people_mesh=True, persons="target")):
        with pytest.raises(ValueError, match=r"people_mesh.*persons|persons.*people_mesh") as e:
            make(**knobs)
        assert "people_mesh" in str(e.value) and "persons" in str(e.value)
    assert make(people_mesh=True, persons="all").people_mesh is True
    assert make(persons="all").people_mesh is False and make().people_mesh is False
    # render_mesh is another knob: on its own it does not turn the people mesh on
    assert make(render_mesh=True).people_mesh is False
