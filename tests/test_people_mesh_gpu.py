"""GPU: the people mesh overlay (csrc/render.hip, pr_render_people; header section r4) against pr_render_overlay (the
reduction property), against the numpy restatement of its contract (tests/raster_people_ref.py) -- face_id bit for bit when the
reference is fed the GPU's own vert_fx --, on its knife edges, between guard bands, and end to end through
Predictor.score_people -> render_people -> __call__ with the people_mesh knob."""
import ctypes as C
import pickle
import sys
import types

import numpy as np
import pytest
import torch

import guard_band as gb
import people_mesh_cases as pmc
import raster_people_ref as rpr
import raster_ref as rr
from poserisk_release_amd import _lib, render, synth, video

pytestmark = pytest.mark.gpu

ALPHA = 0.6
_size_id = lambda s: "%dx%d" % s


def _scene(case, N, H, W, seed):
    return {"soup": pmc.soup, "grid": pmc.grid, "body": pmc.bodies}[case](N, H, W, seed)


def _run(sc, fr, canvas, src_idx, z_step=None, fpart=None, rgb=None, dev="cuda"):
    """-> out, face_id, vert_fx, status, canvas_status as numpy."""
    got = render.overlay_people(torch.from_numpy(fr).to(dev), sc["verts"], sc["faces"], sc["cam"], sc["bboxes"], canvas, src_idx, z_step,
                                scale=pmc.SCALE, face_part=fpart, part_rgb=rgb, alpha=ALPHA, return_face_id=True, return_vert_fx=True,
                                return_status=True, return_canvas_status=True)
    return tuple(t.cpu().numpy() for t in got)


def _tables(sc, P=5):
    return np.arange(len(sc["faces"]), dtype=np.int32) % P, pmc.part_table(len(sc["verts"]), P)


def _check_contract(sc, fr, canvas, src_idx, z_step, fpart, rgb, got):
    """Every output of one call against the reference; returns the reference face_id."""
    out, fid, vfx, st, cst = got
    H, W = fr.shape[1:3]
    want_st, want_cst = rpr.mesh_status(canvas, src_idx, z_step, len(fr))
    np.testing.assert_array_equal(st, want_st)
    np.testing.assert_array_equal(cst, want_cst)
    # the projection: validity equal, coordinates within +-1 of a float64 one, zf shifted by z_step
    want_fx = rpr.vert_fx(sc["verts"], sc["cam"], sc["bboxes"], pmc.SCALE, H, W, z_step, dead=(want_st & 24) != 0)
    np.testing.assert_array_equal(vfx[..., 3], want_fx[..., 3])
    assert np.abs(vfx[..., :3].astype(np.int64) - want_fx[..., :3]).max() <= 1
    keys = rpr.canvas_keys(vfx, sc["faces"], canvas, src_idx, z_step, len(fr), H, W)
    ref, want_fid = rpr.render(fr, sc["verts"], sc["faces"], canvas, src_idx, keys, fpart, rgb, ALPHA)
    np.testing.assert_array_equal(fid, want_fid)
    for m in range(len(src_idx)):
        if want_cst[m]:
            assert not out[m].any()
            continue
        empty = want_fid[m] < 0
        np.testing.assert_array_equal(out[m][empty], fr[src_idx[m]][empty])          # uncovered: the frame, exactly
    assert np.abs(out.astype(np.int32) - ref).max() <= 1                              # covered: +-1 of the float64 blend
    return want_fid


# ---- reduction: one mesh per canvas is pr_render_overlay -------------------------------------------------------------------------
@pytest.mark.parametrize("size", pmc.SIZES, ids=_size_id)
@pytest.mark.parametrize("case", ["soup", "grid", "body"])
def test_one_mesh_per_canvas_is_pr_render_overlay_byte_for_byte(gpu_device, case, size):
    H, W = size
    N = 5
    sc = _scene(case, N, H, W, seed=H + len(case))
    fr = pmc.frames(3, H, W)
    fidx = np.array([2, 0, 1, 1, 0], np.int32)
    fpart, rgb = _tables(sc)
    want = render.overlay(torch.from_numpy(fr).to(gpu_device), sc["verts"], sc["faces"], sc["cam"], sc["bboxes"], scale=pmc.SCALE,
                          frame_idx=fidx, face_part=fpart, part_rgb=rgb, alpha=ALPHA, return_face_id=True, return_vert_fx=True,
                          return_status=True)
    w_out, w_fid, w_vfx, w_st = (t.cpu().numpy() for t in want)
    ident = np.arange(N, dtype=np.int32)
    out, fid, vfx, st, cst = _run(sc, fr, ident, fidx, None, fpart, rgb)
    F = len(sc["faces"])
    local = np.where(fid >= 0, fid - ident[:, None, None] * F, -1)
    assert np.array_equal(out, w_out) and np.array_equal(st, w_st) and np.array_equal(vfx, w_vfx) and not cst.any()
    assert np.array_equal(local, w_fid) and (w_fid >= 0).any()
    # one arbitrary z_step per mesh: a canvas with one mesh does not change
    z = np.array([0, 1, 4097, 1 << 24, 123456], np.int32)
    out_z, fid_z, vfx_z, st_z, _ = _run(sc, fr, ident, fidx, z, fpart, rgb)
    assert np.array_equal(out_z, w_out) and np.array_equal(fid_z, fid) and not st_z.any()
    np.testing.assert_array_equal(vfx_z[..., 2], vfx[..., 2] + np.where(vfx[..., 3] != 0, z[:, None], 0))


# ---- the contract, bit for bit ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", pmc.SIZES, ids=_size_id)
def test_zero_to_sixteen_bodies_a_canvas_with_people_z_step(gpu_device, size):
    H, W = size
    counts = [0, 1, 2, 5, 16]
    canvas = np.random.default_rng(5).permutation(np.repeat(np.arange(5), counts)).astype(np.int32)   # meshes of the canvases interleaved
    sc = pmc.bodies(len(canvas), H, W, seed=H)
    fr = pmc.frames(4, H, W)
    src = np.array([3, 1, 1, 0, 2], np.int32)
    z = render.people_z_step(sc["cam"], sc["bboxes"], pmc.SCALE, H, W)
    assert len(set(z.tolist())) == len(z) and z.min() > 0
    fpart, rgb = _tables(sc, 9)
    got = _run(sc, fr, canvas, src, z, fpart, rgb)
    fid = _check_contract(sc, fr, canvas, src, z, fpart, rgb, got)
    F = len(sc["faces"])
    assert (fid[0] == -1).all() and np.array_equal(got[0][0], fr[3])                      # no mesh: a copy of its frame
    for m, k in enumerate(counts[1:], 1):
        seen = np.unique(fid[m][fid[m] >= 0] // F)
        assert set(seen) <= set(np.nonzero(canvas == m)[0]) and 1 <= len(seen) <= k
    assert len(np.unique(fid[4][fid[4] >= 0] // F)) > 3                                   # several of the 16 are visible
    # who is drawn larger is nearer: where several of the 16 bodies overlap, the one with the most pixels per metre of them wins
    # (almost everywhere: two bodies of nearly one size stand within a body's own depth of each other)
    mine = np.nonzero(canvas == 4)[0]
    cover = np.stack([rr.raster_keys(got[2][n], sc["faces"], H, W) != rr.EMPTY for n in mine])
    nearest = mine[np.argmin(np.where(cover, z[mine][:, None, None], 1 << 30), axis=0)]
    several = cover.sum(0) >= 2
    assert several.sum() > 100 and (fid[4][several] // F == nearest[several]).mean() > 0.9


@pytest.mark.parametrize("size", pmc.SIZES, ids=_size_id)
def test_two_tilted_grids_cross_in_depth(gpu_device, size):
    H, W = size
    slope = 2.0 / W
    sc = pmc.grid(4, H, W, seed=W, tilt=[(2.0, slope), (4.0, -slope), (3.0, 0.0), (2.0, slope)])
    fr = pmc.frames(2, H, W)
    canvas, src = np.array([0, 0, 1, 1], np.int32), np.array([1, 0], np.int32)
    fpart, rgb = _tables(sc)
    fid = _check_contract(sc, fr, canvas, src, None, fpart, rgb, _run(sc, fr, canvas, src, None, fpart, rgb))
    F = len(sc["faces"])
    owner = np.where(fid[0] >= 0, fid[0] // F, -1)
    # the planes meet at x = W / 2: mesh 0 is nearer left of it, mesh 1 right of it (the jittered outlines differ a little)
    left, right = owner[:, :W // 4], owner[:, -(W // 4):]
    assert (left >= 0).any() and (left[left >= 0] == 0).mean() > 0.9
    assert (right >= 0).any() and (right[right >= 0] == 1).mean() > 0.9
    # canvas 1: the flat plane at 3 m and the tilted one, 2 m .. 4 m, meet at x = W / 2; half a metre of z_step moves that to W / 4
    band = lambda f: np.where(f >= 0, f // F, -1)[:, W // 3:W // 2 - 3]
    assert (band(fid[1])[band(fid[1]) >= 0] == 3).mean() > 0.9
    z = np.array([0, 0, 0, 2048], np.int32)
    fid = _check_contract(sc, fr, canvas, src, z, fpart, rgb, _run(sc, fr, canvas, src, z, fpart, rgb))
    assert (band(fid[1])[band(fid[1]) >= 0] == 2).mean() > 0.9 and set(np.unique(fid[1][fid[1] >= 0] // F)) == {2, 3}
    assert np.array_equal(np.where(fid[0] >= 0, fid[0] // F, -1), owner)


@pytest.mark.parametrize("size", pmc.SIZES, ids=_size_id)
def test_frame_spanning_faces_of_two_meshes_overlap(gpu_device, size):
    H, W = size
    sc = pmc.spanning(5, H, W, seed=H)
    fr = pmc.frames(2, H, W)
    canvas, src = np.array([1, 0, 1, 0, 1], np.int32), np.array([0, 1], np.int32)
    fpart, rgb = _tables(sc, 3)
    fid = _check_contract(sc, fr, canvas, src, None, fpart, rgb, _run(sc, fr, canvas, src, None, fpart, rgb))
    for m in (0, 1):
        assert len(np.unique(fid[m][fid[m] >= 0] // 4)) >= 2 and (fid[m] >= 0).mean() > 0.5


def test_soup_meshes_share_canvases(gpu_device):
    H, W = pmc.SIZES[0]
    sc = pmc.soup(6, H, W, seed=2)
    fr = pmc.frames(3, H, W)
    canvas, src = np.array([0, 2, 0, 2, 2, 0], np.int32), np.array([0, 1, 2], np.int32)
    z = np.array([0, 500, 300, 0, 12000, 300], np.int32)
    fpart, rgb = _tables(sc)
    fid = _check_contract(sc, fr, canvas, src, z, fpart, rgb, _run(sc, fr, canvas, src, z, fpart, rgb))
    assert (fid[1] == -1).all() and len(np.unique(fid[0][fid[0] >= 0] // len(sc["faces"]))) == 3


# ---- knife edges -----------------------------------------------------------------------------------------------------------------
def _twice(sc):
    return {k: (v if k == "faces" else np.concatenate([v[:1], v[:1]])) for k, v in sc.items()}


@pytest.mark.parametrize("case", ["soup", "body"])
def test_depth_ties_go_to_the_lower_mesh_and_one_step_decides(gpu_device, case):
    H, W = pmc.SIZES[1]                                                   # the smallest body here is about 30 x 9 px: > 200 px covered
    sc = _twice(_scene(case, 1, H, W, seed=3))
    fr = pmc.frames(1, H, W)
    F = len(sc["faces"])
    both, src = np.zeros(2, np.int32), np.zeros(1, np.int32)
    alone = _run({k: (v if k == "faces" else v[:1]) for k, v in sc.items()}, fr, both[:1], src)
    for z, owner in ((None, 0), ((5, 5), 0), ((8, 7), 1), ((7, 8), 0)):
        out, fid, _, st, _ = _run(sc, fr, both, src, None if z is None else np.array(z, np.int32))
        assert not st.any() and (fid[0] >= 0).sum() > 50
        assert np.array_equal(fid[0] >= 0, alone[1][0] >= 0) and (fid[0][fid[0] >= 0] // F == owner).all(), (z, owner)
        # the twin's faces are the same faces: the picture is the one mesh's
        assert np.array_equal(np.where(fid[0] >= 0, fid[0] % F, -1), alone[1][0]) and np.array_equal(out, alone[0])


def test_z_step_range_canvas_range_and_bad_src_idx(gpu_device):
    H, W = pmc.SIZES[0]
    sc = pmc.grid(8, H, W, seed=6)
    fr = pmc.frames(2, H, W)
    M = 4
    src = np.array([1, 0, 5, 0], np.int32)                                # canvas 2: no such frame
    canvas = np.array([0, 0, 0, 0, -1, M, 2, 3], np.int32)
    z = np.array([0, 1 << 24, -1, (1 << 24) + 1, 0, 0, 0, 0], np.int32)
    fpart, rgb = _tables(sc)
    got = _run(sc, fr, canvas, src, z, fpart, rgb)
    out, fid, vfx, st, cst = got
    assert st.tolist() == [0, 0, 16, 16, 8, 8, 1, 0] and cst.tolist() == [0, 0, 1, 0]
    _check_contract(sc, fr, canvas, src, z, fpart, rgb, got)
    F = len(sc["faces"])
    owners = set(np.unique(fid[fid >= 0] // F).tolist())                   # mesh 1, 4096 m behind mesh 0, shows at most past its outline
    assert {0, 7} <= owners <= {0, 1, 7}
    assert not vfx[2:6].any() and vfx[6, :, 3].all()
    assert not out[2].any() and (fid[2] == -1).all()                      # the bad canvas only
    assert np.array_equal(out[1], fr[0]) and (fid[3] >= 0).any()
    # z_step 2^24 alone on a canvas draws as z_step 0 does
    one = {k: (v if k == "faces" else v[1:2]) for k, v in sc.items()}
    a = _run(one, fr, np.zeros(1, np.int32), src[:1], np.array([1 << 24], np.int32), fpart, rgb[1:2])
    b = _run(one, fr, np.zeros(1, np.int32), src[:1], np.array([0], np.int32), fpart, rgb[1:2])
    assert not a[3].any() and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and (a[1] >= 0).any()
    assert int(a[2][..., 2].max()) < (1 << 25)


@pytest.mark.parametrize("size", pmc.SIZES, ids=_size_id)
def test_a_uniform_shift_of_a_canvas_changes_no_byte(gpu_device, size):
    H, W = size
    sc = pmc.bodies(7, H, W, seed=W)
    fr = pmc.frames(2, H, W)
    canvas, src = np.array([0, 1, 0, 0, 1, 0, 1], np.int32), np.array([1, 0], np.int32)
    z = render.people_z_step(sc["cam"], sc["bboxes"], pmc.SCALE, H, W)
    fpart, rgb = _tables(sc, 9)
    base = _run(sc, fr, canvas, src, z, fpart, rgb)
    shift = np.where(canvas == 0, 777, 31)                                 # one shift per canvas
    moved = _run(sc, fr, canvas, src, (z + shift).astype(np.int32), fpart, rgb)
    assert np.array_equal(base[0], moved[0]) and np.array_equal(base[1], moved[1]) and (base[1] >= 0).any()
    np.testing.assert_array_equal(moved[2][..., 2] - base[2][..., 2], np.where(base[2][..., 3] != 0, shift[:, None], 0))


# ---- batch independence ----------------------------------------------------------------------------------------------------------
def test_a_canvas_does_not_depend_on_the_rest_of_the_batch(gpu_device):
    H, W = pmc.SIZES[1]
    sc = pmc.bodies(9, H, W, seed=21)
    fr = pmc.frames(3, H, W)
    z = render.people_z_step(sc["cam"], sc["bboxes"], pmc.SCALE, H, W)
    fpart, rgb = _tables(sc, 9)
    F = len(sc["faces"])
    pick = lambda idx: ({k: (v if k == "faces" else v[idx]) for k, v in sc.items()}, z[idx], rgb[idx])
    mine = np.array([0, 1, 2, 3])                                         # the canvas under test: meshes 0..3 over frame 1

    def local(fid, where):
        """face_id with mesh indices mapped back to positions within `mine` (-1: none; -2: a mesh that is not ours)."""
        n, f = fid // F, fid % F
        pos = np.full(fid.shape, -2, np.int64)
        for k, w in enumerate(where):
            pos[n == w] = k
        return np.where(fid < 0, -1, pos * F + f)
    s, zz, cc = pick(mine)
    alone = _run(s, fr, np.zeros(4, np.int32), np.array([1], np.int32), zz, fpart, cc)
    want_out, want_fid = alone[0][0], local(alone[1][0], range(4))
    assert (want_fid >= 0).any() and len(np.unique(want_fid[want_fid >= 0] // F)) > 1
    # in the middle of a batch, its meshes behind another canvas's
    order = np.array([4, 5, 0, 1, 2, 3, 6, 7, 8])
    s, zz, cc = pick(order)
    mid = _run(s, fr, np.array([0, 0, 1, 1, 1, 1, 2, 2, 2], np.int32), np.array([0, 1, 2], np.int32), zz, fpart, cc)
    assert np.array_equal(mid[0][1], want_out) and np.array_equal(local(mid[1][1], [2, 3, 4, 5]), want_fid)
    # its meshes interleaved with another canvas's (their relative order kept)
    order = np.array([4, 0, 5, 1, 6, 2, 7, 3, 8])
    s, zz, cc = pick(order)
    mix = _run(s, fr, np.array([0, 1, 0, 1, 0, 1, 0, 1, 0], np.int32), np.array([2, 1], np.int32), zz, fpart, cc)
    assert np.array_equal(mix[0][1], want_out) and np.array_equal(local(mix[1][1], [1, 3, 5, 7]), want_fid)


# ---- argument errors, N = 0, M = 0, guard bands ----------------------------------------------------------------------------------
def _dev_case(gpu_device, case="grid", N=3, M=2, seed=8):
    H, W = pmc.SIZES[0]
    sc = _scene(case, N, H, W, seed)
    fr = pmc.frames(2, H, W)
    fpart, rgb = _tables(sc)
    host = dict(verts=sc["verts"], faces=sc["faces"], cam=sc["cam"], bboxes=sc["bboxes"], frames=fr,
                canvas=np.array([1, 0, 1], np.int32)[:N], src_idx=np.array([1, 0], np.int32)[:M], z_step=np.array([40, 0, 9], np.int32)[:N],
                face_part=fpart, part_rgb=rgb)
    return sc, host, {k: torch.from_numpy(np.ascontiguousarray(v)).to(gpu_device) for k, v in host.items()}


def test_every_argument_error_and_the_empty_calls(gpu_device):
    lib = _lib.load()
    H, W = pmc.SIZES[0]
    sc, host, t = _dev_case(gpu_device)
    N, M, V, F = 3, 2, sc["verts"].shape[1], len(sc["faces"])
    out = torch.full((M, H, W, 3), 7, dtype=torch.uint8, device=gpu_device)
    status = torch.full((N,), -7, dtype=torch.int32, device=gpu_device)
    nb = lib.pr_render_people_workspace_bytes(N, M, V, F, H, W)
    assert nb >= M * H * W * 8 + N * V * 16 + 2 * N * F * 4
    ws = torch.empty((nb,), dtype=torch.uint8, device=gpu_device)
    stream = torch.cuda.current_stream().cuda_stream

    def call(ws_bytes=nb, workspace=ws.data_ptr(), **over):
        v = dict({k: x.data_ptr() for k, x in t.items()}, out=out.data_ptr(), face_id=None, vert_fx=None, status=status.data_ptr(),
                 canvas_status=None, N=N, M=M, V=V, F=F, P=5, n_frames=2, H=H, W=W, bgr=0, scale=pmc.SCALE, alpha=ALPHA)
        v.update(over)
        rc = lib.pr_render_people(C.byref(_lib.RenderPeopleArgs(**v)), workspace, ws_bytes, stream)
        return rc, lib.pr_last_error().decode()
    for over, word in ((dict(N=-1), "N = -1"), (dict(M=-1), "M = -1"), (dict(frames=None), "null"), (dict(out=None), "null"),
                       (dict(verts=None), "null"), (dict(faces=None), "null"), (dict(cam=None), "null"), (dict(bboxes=None), "null"),
                       (dict(canvas=None), "null"), (dict(face_part=None), "null"), (dict(part_rgb=None), "null"),
                       (dict(workspace=None), "null workspace"), (dict(ws_bytes=nb - 1), "workspace of"), (dict(n_frames=0), "n_frames"),
                       (dict(H=0), "1..4096"), (dict(W=4097), "1..4096"), (dict(V=2), "V=2"), (dict(F=0), "F=0"), (dict(P=0), "P=0"),
                       (dict(scale=0.0), "scale"), (dict(alpha=1.5), "alpha"), (dict(alpha=-0.1), "alpha"),
                       (dict(src_idx=None, M=3), "without src_idx")):
        rc, msg = call(**over)
        assert rc == -1 and word in msg and "pr_render_people" in msg, (over, rc, msg)       # PR_ERR_INVALID
    assert lib.pr_render_people(None, ws.data_ptr(), nb, stream) == -1
    assert lib.pr_render_people_workspace_bytes(N, 0, V, F, H, W) == 0 and lib.pr_render_people_workspace_bytes(-1, M, V, F, H, W) == 0
    assert call(M=0, out=None, frames=None, workspace=None, ws_bytes=0)[0] == 0          # M = 0: PR_OK, nothing looked at
    torch.cuda.synchronize()
    assert (out == 7).all() and (status == -7).all()                                     # no device work happened
    # N = 0 copies the frames; the mesh arguments are not looked at
    nb0 = lib.pr_render_people_workspace_bytes(0, M, 0, 0, H, W)
    assert 0 < nb0 <= nb
    assert call(N=0, verts=None, faces=None, cam=None, bboxes=None, canvas=None, z_step=None, face_part=None, part_rgb=None, status=None,
                V=0, F=0, P=0, ws_bytes=nb0)[0] == 0
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), host["frames"][[1, 0]]) and (status == -7).all()
    assert call()[0] == 0                                                                # and the call these were derived from is valid
    torch.cuda.synchronize()
    assert status.cpu().tolist() == [0, 0, 0] and (out.cpu().numpy() != host["frames"][[1, 0]]).any()
    # the wrapper: N = 0 and M = 0
    fr = t["frames"]
    none = render.overlay_people(fr, np.zeros((0, V, 3), np.float32), sc["faces"], np.zeros((0, 3)), np.zeros((0, 4)), np.zeros(0, np.int32),
                                 host["src_idx"])
    assert np.array_equal(none.cpu().numpy(), host["frames"][[1, 0]])
    assert render.overlay_people(fr, sc["verts"], sc["faces"], sc["cam"], sc["bboxes"], host["canvas"], np.zeros(0, np.int32)).shape == (0, H, W, 3)


def test_every_tensor_stays_inside_its_guard_bands(gpu_device):
    """Outputs between canary guards, inputs between guards of NaN / 255 / 0x7fffffff (tests/guard_band.py); the soups hold
    faces larger than the frame and faces across every frame edge, and the workspace is exactly
    pr_render_people_workspace_bytes long.  (A vertex coordinate may be the int32 canary, -7, in its own right: the comparison
    with an unguarded run says whether every word was written.)"""
    H, W = pmc.SIZES[0]
    sc, host, t = _dev_case(gpu_device, "soup")
    N, M, V, F = 3, 2, sc["verts"].shape[1], len(sc["faces"])
    lib = _lib.load()
    nb = lib.pr_render_people_workspace_bytes(N, M, V, F, H, W)

    def call(i, o):
        ws = torch.empty((nb,), dtype=torch.uint8, device=gpu_device)
        args = _lib.RenderPeopleArgs(i["verts"].data_ptr(), i["faces"].data_ptr(), i["cam"].data_ptr(), i["bboxes"].data_ptr(),
                                     i["frames"].data_ptr(), i["canvas"].data_ptr(), i["src_idx"].data_ptr(), i["z_step"].data_ptr(),
                                     i["face_part"].data_ptr(), i["part_rgb"].data_ptr(), o["out"].data_ptr(), o["face_id"].data_ptr(),
                                     o["vert_fx"].data_ptr(), o["status"].data_ptr(), o["canvas_status"].data_ptr(), N, M, V, F, 5, 2, H, W,
                                     0, pmc.SCALE, ALPHA)
        _lib.check(lib.pr_render_people(C.byref(args), ws.data_ptr(), nb, torch.cuda.current_stream().cuda_stream), "pr_render_people")
    got = gb.run_guarded(call, t, {"out": ((M, H, W, 3), torch.uint8), "face_id": ((M, H, W), torch.int32), "vert_fx": ((N, V, 4), torch.int32),
                                   "status": ((N,), torch.int32), "canvas_status": ((M,), torch.int32)}, may_hold_canary=("out", "vert_fx"))
    want = _run(sc, host["frames"], host["canvas"], host["src_idx"], host["z_step"], host["face_part"], host["part_rgb"])
    for name, w in zip(("out", "face_id", "vert_fx", "status", "canvas_status"), want):
        assert np.array_equal(got[name].cpu().numpy(), w), name
    _check_contract(sc, host["frames"], host["canvas"], host["src_idx"], host["z_step"], host["face_part"], host["part_rgb"], want)


# ---- the Predictor: persons='all' with the people_mesh knob -----------------------------------------------------------------------
N_FRAMES = 24


@pytest.fixture(scope="module")
def clip():
    """24 frames of 160 x 120 and three tracks of 24, 17 and 9 frames whose boxes overlap, largest first."""
    rng = np.random.default_rng(9)
    frames = rng.integers(0, 256, (N_FRAMES, 120, 160, 3), dtype=np.uint8)
    tr = {}
    for pid, (first, n, w, h, x) in {5: (0, 24, 50, 100, 40), 2: (4, 17, 40, 80, 85), 11: (15, 9, 30, 60, 120)}.items():
        tr[pid] = {'bbox': np.stack([np.array([x + i, 60 - i % 3, w, h], np.float32) for i in range(n)]), 'frames': np.arange(first, first + n)}
    return frames, tr


def _predictor(gpu_device, score_type="REBA", **knobs):
    from poserisk_release_amd import dropin
    dropin.install()
    from core import base
    from models import hmr
    from smpl import SMPL
    model = hmr()
    model.load_state_dict(synth.hmr_state_dict(seed=1), strict=False)
    sm = synth.smpl_model(V=6890, seed=2)
    sm["f"] = synth.genus0_mesh(6890)[1]
    smpl = SMPL(models={"neutral": sm}, device=gpu_device)
    args = types.SimpleNamespace(gpu="0", type=score_type, debug=False, debug_joints="", debug_frame=-1, **knobs)
    return base.Predictor(args, spin_model=model, smpl_model=smpl, batch_size=16), sm


@pytest.fixture(scope="module")
def scored(gpu_device, clip):
    """One Predictor with the knob on and what its score_people returns for the clip (shared, left unchanged)."""
    pred, sm = _predictor(gpu_device, persons="all", people_mesh=True, gpu_video=True, video_codec="png")
    frames, tr = clip
    return pred, sm, pred.score_people(frames, tr, synth.EXAMPLE_INFO)


def test_score_people_returns_every_persons_smpl_parameters(gpu_device, clip, scored):
    frames, tr = clip
    pred, _, people = scored
    assert people["ids"] == [5, 2, 11]
    for p, pid in enumerate(people["ids"]):
        alone = pred.score_frames(frames, {pid: tr[pid]}, synth.EXAMPLE_INFO, with_smpl_params=True)
        got = people["people"][p]
        assert list(got) == list(alone) and {"rotmat", "betas", "cam", "add_info", "bbox_scale"} <= set(got)
        for k in alone:
            if k == "reba":
                (fa, sa, la, aa), (fb, sb, lb, ab) = got[k], alone[k]
                assert np.array_equal(np.array(fa), np.array(fb), equal_nan=True) and np.array_equal(sa, sb) and np.array_equal(la, lb) and aa == ab
            elif k in ("add_info", "bbox_scale"):
                assert got[k] == alone[k]
            else:
                assert np.asarray(got[k]).dtype == np.asarray(alone[k]).dtype and np.array_equal(got[k], alone[k]), (pid, k)
    # off, by argument or by knob: the dict is what it was
    plain = pred.score_people(frames, tr, synth.EXAMPLE_INFO, with_smpl_params=False)
    off, _ = _predictor(gpu_device, persons="all")
    for some in (plain, off.score_people(frames, tr, synth.EXAMPLE_INFO)):
        assert set(some) == {"people", "ids", "frames_total"}
        assert all(list(o) == ["result", "joint_cam", "debug_result", "reba", "frames", "bboxes"] for o in some["people"])
        assert all(np.array_equal(o["result"], w["result"]) for o, w in zip(some["people"], people["people"]))
    with pytest.raises(ValueError, match="with_smpl_params"):
        list(off.render_people(plain, frames, "REBA"))
    with pytest.raises(NotImplementedError, match="render_mesh"):
        _predictor(gpu_device, render_mesh=True)[0].score_people(frames, tr, synth.EXAMPLE_INFO)


def _by_hand(pred, sm, people, frames, title, gpu_device):
    """overlay_people on the arrays score_people returned: every (person, frame) row a mesh, every video frame a canvas."""
    from poserisk_release_amd import ops
    rows = [(p, r) for p, o in enumerate(people["people"]) for r in range(len(o["frames"]))]
    cat = lambda k: np.concatenate([o[k] for o in people["people"]])
    rot = torch.from_numpy(cat("rotmat")).to(gpu_device)
    aa, eul, _ = ops.pose_to_euler(rot)
    verts, _ = pred.smpl_model.layer['neutral'](aa.reshape(len(rows), 72), torch.from_numpy(cat("betas")).to(gpu_device))
    packed = ops.reba(eul, synth.EXAMPLE_INFO[title]).cpu().numpy()
    H, W = frames.shape[1:3]
    z = render.people_z_step(cat("cam"), cat("bboxes"), 1.2, H, W)
    return render.overlay_people(torch.from_numpy(frames).to(gpu_device), verts, sm["f"], cat("cam"), cat("bboxes"),
                                 cat("frames").astype(np.int32), np.arange(len(frames), dtype=np.int32), z, scale=1.2,
                                 face_part=render.face_parts(sm["weights"], sm["f"], title), part_rgb=render.part_colours(packed, title),
                                 alpha=0.6, return_face_id=True)


def test_render_people_is_overlay_people_on_the_returned_arrays(gpu_device, clip, scored):
    frames, tr = clip
    pred, sm, people = scored
    got = list(pred.render_people(people, frames, "REBA"))
    assert [len(n) for n, _ in got] == [16, 8] and np.concatenate([n for n, _ in got]).tolist() == list(range(N_FRAMES))
    imgs = np.concatenate([i.cpu().numpy() for _, i in got])
    want, fid = _by_hand(pred, sm, people, frames, "REBA", gpu_device)
    assert imgs.shape == (N_FRAMES, 120, 160, 3) and imgs.tobytes() == want.cpu().numpy().tobytes()
    # frame 20 shows all three people, in people_tracks order: mesh rows of persons 0, 1, 2
    fid = fid.cpu().numpy()
    F = len(sm["f"])
    starts = np.cumsum([0] + [len(o["frames"]) for o in people["people"]])
    owners = np.unique(np.searchsorted(starts, fid[20][fid[20] >= 0] // F, side="right") - 1)
    assert owners.tolist() == [0, 1, 2]
    assert np.array_equal(imgs[2][fid[2] < 0], frames[2][fid[2] < 0]) and (fid[2] >= 0).any()


def test_people_mesh_end_to_end(gpu_device, clip, scored, tmp_path, monkeypatch, capsys):
    from PIL import Image
    monkeypatch.setitem(sys.modules, "cv2", None)
    frames, tr = clip
    src = tmp_path / "clip"
    src.mkdir()
    np.save(src / "frames.npy", frames)
    with open(src / "tracking.pkl", "wb") as f:
        pickle.dump(tr, f)
    pred, sm, people = scored
    out = pred(str(src), "", str(tmp_path / "mesh"))
    plain, _ = _predictor(gpu_device, persons="all", gpu_video=True, video_codec="png")
    plain(str(src), "", str(tmp_path / "plain"))
    assert not (tmp_path / "plain" / "REBA_people_mesh").exists()
    imgs = np.concatenate([i.cpu().numpy() for _, i in pred.render_people(out["people"], frames, "REBA")])
    read = lambda p: np.asarray(Image.open(p).convert("RGB"))
    names = ['{0:09d}.png'.format(i) for i in range(N_FRAMES)]
    assert sorted(p.name for p in (tmp_path / "mesh" / "REBA_people_mesh").iterdir()) == names
    for i in (0, 5, 20, 23):
        assert np.array_equal(read(tmp_path / "mesh" / "REBA_people_mesh" / names[i]), imgs[i]), i
    # <TITLE>_people: boxes and tags over those images
    ppl = []
    for pid, o in zip(out["people"]["ids"], out["people"]["people"]):
        acts = [pred.reba.action_level(s) for s in o["reba"][1]]
        ppl.append(dict(id=pid, frames=o["frames"], bboxes=o["bboxes"], scores=o["reba"][1], levels=[a[0] for a in acts], names=[a[1] for a in acts]))
    dst_h, dst_w, panel_w = video.canvas_size(120, 160)
    draw = video.people_draw_list("REBA", N_FRAMES, ppl, dst_h, dst_w, 120, 160)
    want = torch.cat(list(video.people_frames(torch.from_numpy(imgs).to(gpu_device), draw, 16))).cpu().numpy()
    for i in (0, 5, 20, 23):
        assert np.array_equal(read(tmp_path / "mesh" / "REBA_people" / names[i]), want[i]), i
    a, b = read(tmp_path / "mesh" / "REBA_people" / names[20]), read(tmp_path / "plain" / "REBA_people" / names[20])
    assert (a[:, :dst_w] != b[:, :dst_w]).any() and np.array_equal(a[:, dst_w:], b[:, dst_w:])
    # every other file is what the run without the knob writes
    for p in (tmp_path / "plain").rglob("*"):
        if p.is_file() and p.parent.name != "REBA_people":
            assert (tmp_path / "mesh" / p.relative_to(tmp_path / "plain")).read_bytes() == p.read_bytes(), p
    # without gpu_video: one line, no mesh
    capsys.readouterr()
    cpu, _ = _predictor(gpu_device, persons="all", people_mesh=True)
    cpu(str(src), "", str(tmp_path / "cpu"))
    said = capsys.readouterr().out
    assert said.count("people mesh") == 1 and "gpu_video" in said and not (tmp_path / "cpu" / "REBA_people_mesh").exists()
