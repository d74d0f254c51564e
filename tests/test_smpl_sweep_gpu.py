"""The SMPL kernels (csrc/smpl.hip) against a float64 restatement, over every model the handle accepts.

The older SMPL tests compare float32 with float32 at atol 1e-5, on models with exactly 4 (or 24) weights per vertex, 10 shape
coefficients, SMPL's own tree, small angles and no centre joint.  Here, for each case of tests/smpl_cases.py (every skinning
instantiation x every vertex-count class: tile edges and the first vertex behind a group of 8 tiles; 1 to 24 weights per
vertex with ragged and empty rows; 0 to 16 shape coefficients; chain, star and random trees; a centre joint; a translation
absent, zero and non-zero; angles up to N(0, 3^2), whole turns and the vectors around the 1e-8 of the norm; batches around the
16-frame group and the max_batch chunk edge), `forward` and `joint_cam(return_verts=True)` must be within

    2 * e_f32 + spacing(float32(max |value|))

of tests/smpl_ref64.py, where e_f32 is the distance of the float32 oracle (oracle/smpl_ref.py) from the same float64 values
on the same case and output: the bound comes from float32 arithmetic in another order, never from the kernel.  Every case
runs once between guard bands (tests/guard_band.py) and once on plain tensors, with equal bits, and once more under the
library's internal fence in both modes.

Bits: the register-tiled kernel and the wave-split one agree wherever the first is eligible; a frame's bits depend neither
on the batch nor on its slot in it (the slots around the 16-frame group edge and the chunk edge); a NaN pose stays in its
frame.  The reference's quirk that values whose float32 squares underflow count as "not given" (smpl_layer.py:87,148) is
held to the reference's own fixture, also when the call is split into chunks.
"""
import numpy as np
import pytest
import torch

import smpl_cases as sc
import smpl_ref64
import test_guard_band_gpu as tg
import test_internal_fence_gpu as tf
from conftest import golden, measured
from oracle import smpl_ref
from poserisk_release_amd import _lib
from poserisk_release_amd.smpl_layer import SMPLLayer

pytestmark = pytest.mark.gpu

F32 = torch.float32
OUTPUTS = ("verts", "joints", "joint_cam", "joint_cam verts")
_WORST = {}          # (variant, output) -> the family's largest e_gpu / e_f32 so far; (variant, output, "bound") -> e_gpu / bound


def _env(mp, tile):
    if tile is None:
        mp.delenv("POSERISK_SMPL_TILE", raising=False)
    else:
        mp.setenv("POSERISK_SMPL_TILE", tile)             # read by pr_smpl_create


def _layer(mp, dev, model, handle, center_idx=None, max_batch=None):
    mb, tile = sc.HANDLES[handle]
    _env(mp, tile)
    layer = SMPLLayer(model, center_idx=center_idx, device=dev, max_batch=max_batch or mb)
    layer._ensure()
    return layer


def _dev(dev, *arrays):
    return [None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrays]


def _run(layer, dev, pose, betas, trans):
    """forward and joint_cam on plain tensors -> {output: tensor}."""
    p, b, t = _dev(dev, pose, betas, trans)
    v, j = layer(p, b, t)
    jc, v2 = layer.joint_cam(p.reshape(-1, 24, 3).clone(), return_verts=True)
    return dict(zip(OUTPUTS, (v, j, jc, v2)))


def _record(variant, output, e_gpu, e_f32, bound):
    """The family's largest e_gpu / bound, and its largest e_gpu / e_f32 with the two errors it was made of."""
    unit = "mm" if output == "joint_cam" else "m"
    use = _WORST[variant, output, "bound"] = max(e_gpu / bound, _WORST.get((variant, output, "bound"), 0.0))
    measured(f"smpl_sweep {variant} {output} largest e_gpu/bound", use, 1.0)
    if e_f32 > 0 and e_gpu / e_f32 >= _WORST.get((variant, output), 0.0):
        _WORST[variant, output] = e_gpu / e_f32
        measured(f"smpl_sweep {variant} {output} largest e_gpu/e_f32", e_gpu / e_f32)
        measured(f"smpl_sweep {variant} {output} largest e_gpu/e_f32: e_gpu", e_gpu, unit=unit)
        measured(f"smpl_sweep {variant} {output} largest e_gpu/e_f32: e_f32", e_f32, unit=unit)


@pytest.mark.parametrize("name", [c.name for c in sc.CASES])
def test_sweep(gpu_device, monkeypatch, name):
    c = sc.BY_NAME[name]
    model, (pose, betas, trans), r64, o32 = sc.references(name)
    layer = _layer(monkeypatch, gpu_device, model, c.handle, c.center_idx)
    given = {k: a for k, a in (("pose", pose), ("betas", betas), ("trans", trans)) if a is not None}

    def forward(i, o):
        v, j = layer(i["pose"], i.get("betas"), i.get("trans"), out=None if o is None else (o["verts"], o["joints"]))
        return {"verts": v, "joints": j}

    got = tg.guarded(forward, dict(zip(given, _dev(gpu_device, *given.values()))),
                     {"verts": ((c.B, c.V, 3), F32), "joints": ((c.B, 24, 3), F32)})

    def joint_cam(i, o):
        jc, v = layer.joint_cam(i["aa"], return_verts=True, out=None if o is None else (o["joint_cam"], o["joint_cam verts"]))
        return {"joint_cam": jc, "joint_cam verts": v}

    # (joint_cam overwrites the root rows of its input in place, the reference's quirk: the one input a kernel may write)
    got.update(tg.guarded(joint_cam, {"aa": _dev(gpu_device, pose.reshape(c.B, 24, 3))[0]},
                          {"joint_cam": ((c.B, 24, 3), F32), "joint_cam verts": ((c.B, c.V, 3), F32)}, mutated=("aa",)))
    failures = []
    for k in OUTPUTS:
        ok, e_gpu, e_f32, bound = sc.check(got[k].cpu().numpy(), r64[k], o32[k])
        print(f"[sweep] {name} {k}: e_gpu {e_gpu:.3e} e_f32 {e_f32:.3e} bound {bound:.3e}")
        _record(sc.variant(c), k, e_gpu, e_f32, bound)
        if not ok:
            failures.append(f"{k}: e_gpu {e_gpu:.3e} > 2 * e_f32 ({e_f32:.3e}) + one spacing = {bound:.3e}")
    assert not failures, f"{name}: " + "; ".join(failures)
    # root-relative: the root's own row is (x * 1000) - (x * 1000), exactly 0 in the reference; a contracted
    # fma(x, 1000, -(x * 1000)) leaves the product's rounding error there (found by the one-vertex cases of this sweep)
    assert float(got["joint_cam"][:, 0].abs().max()) == 0.0


@pytest.mark.parametrize("name", [c.name for c in sc.CASES if sc.tile_eligible(c)])
def test_tile_switch_leaves_the_bits(gpu_device, monkeypatch, name):
    """POSERISK_SMPL_TILE = 1 and = 0 on every case the register-tiled kernel is eligible for: equal verts and joints."""
    c = sc.BY_NAME[name]
    model, (pose, betas, trans), _, _ = sc.references(name)
    outs = [_run(_layer(monkeypatch, gpu_device, model, h, c.center_idx), gpu_device, pose, betas, trans) for h in ("tile", "split")]
    for k in OUTPUTS:
        assert torch.equal(outs[0][k], outs[1][k]), f"{name}: {k} differs between the tiled and the wave-split kernel"


@pytest.fixture(scope="module")
def body85():
    """85 vertices (two 84-vertex tiles, five 21-vertex ones), up to 4 weights: a model all three variants take."""
    return sc.make_model(85, 10, 4, "smpl", seed=77)


@pytest.mark.parametrize("handle", list(sc.HANDLES))
def test_a_frames_bits_do_not_depend_on_the_batch(gpu_device, monkeypatch, body85, handle):
    """One frame alone, and the same frame at the slots that bracket the 16-frame group edge and the max_batch chunk edge
    of a call of 2 * max_batch + 3 frames whose other frames differ: the same bits."""
    mb = sc.HANDLES[handle][0]
    B = 2 * mb + 3
    rng = np.random.default_rng(5)
    pose = rng.normal(0, 1.0, (B, 72)).astype(np.float32)
    betas = rng.normal(0, 1.0, (B, 10)).astype(np.float32)
    trans = rng.normal(0, 0.3, (B, 3)).astype(np.float32)
    slots = sorted({0, 15, 16, 17, mb - 1, mb, mb + 1, 2 * mb - 1, 2 * mb, B - 1})
    for a in (pose, betas, trans):
        a[slots] = a[0]
    layer = _layer(monkeypatch, gpu_device, body85, handle, center_idx=None)
    alone = _run(layer, gpu_device, pose[:1], betas[:1], trans[:1])
    batch = _run(layer, gpu_device, pose, betas, trans)
    for k in OUTPUTS:
        for s in slots:
            assert torch.equal(batch[k][s], alone[k][0]), f"{handle}: {k} of the frame at slot {s} of {B} differs from the frame alone"
        assert not torch.equal(batch[k][1], alone[k][0])


@pytest.mark.parametrize("handle", list(sc.HANDLES))
def test_a_nan_pose_stays_in_its_frame(gpu_device, monkeypatch, body85, handle):
    mb = sc.HANDLES[handle][0]
    B = mb + 3
    rng = np.random.default_rng(6)
    pose = rng.normal(0, 1.0, (B, 72)).astype(np.float32)
    betas = rng.normal(0, 1.0, (B, 10)).astype(np.float32)
    layer = _layer(monkeypatch, gpu_device, body85, handle, center_idx=12)
    clean = _run(layer, gpu_device, pose, betas, None)
    bad = pose.copy()
    bad[5, 30] = np.nan                     # joint 10 of frame 5 (not the root: joint_cam overwrites that)
    bad[mb, 3:] = np.nan                    # every other joint of the first frame of the second chunk
    dirty = _run(layer, gpu_device, bad, betas, None)
    keep = [f for f in range(B) if f not in (5, mb)]
    for k in OUTPUTS:
        assert torch.equal(dirty[k][keep], clean[k][keep]), f"{handle}: a NaN pose changed {k} of another frame"
        # (the NaNs did arrive: a leaf joint's rotation reaches every vertex through the pose blend but no joint position)
        assert bool(torch.isnan(dirty[k][mb]).any()) and (bool(torch.isnan(dirty[k][5]).any()) or "verts" not in k)


# ---- values whose float32 squares underflow count as "not given" (smpl_layer.py:87,148) ------------------------------------

@pytest.mark.parametrize("max_batch", [17, 2])       # 2: the three frames are two chunks, the decision is the call's
@pytest.mark.parametrize("name", ["tiny_betas_tiny_trans", "tiny_betas", "tiny_trans"])
def test_tiny_values_follow_the_references_fixture(gpu_device, monkeypatch, name, max_batch):
    g = golden("smpl_sweep.npz")
    spec, model = sc.FIXTURES[name], sc.fixture_model(name)
    pose, betas, trans = g[f"{name}_pose"], g[f"{name}_betas"], g[f"{name}_trans"]
    layer = _layer(monkeypatch, gpu_device, model, "tile", spec["center_idx"], max_batch=max_batch)
    v, j = layer(*_dev(gpu_device, pose, betas, trans))
    for k, got in (("verts", v), ("joints", j)):
        d = np.abs(got.cpu().numpy() - g[f"{name}_{k}"]).max()
        measured(f"smpl_sweep fixture {name} max_batch {max_batch} {k}", d, 2e-6, "m")
        assert d <= 2e-6, f"{name} {k}: {d:.3e} from the reference's output (2.1 cm is the other branch)"


@pytest.mark.parametrize("which", ["betas", "trans"])
def test_the_decision_is_over_the_whole_call(gpu_device, monkeypatch, which):
    """Four frames in chunks of two; the first chunk's betas (trans) are all 1e-23, the second chunk's are not: the tensor
    as a whole is not zero, so the first chunk's tiny values are used as they are, as in the reference."""
    model = sc.fixture_model("tiny_betas")                       # non-zero model betas
    rng = np.random.default_rng(8)
    pose = rng.normal(0, 0.5, (4, 72)).astype(np.float32)
    betas = rng.normal(0, 1.0, (4, 10)).astype(np.float32)
    trans = rng.normal(0, 0.3, (4, 3)).astype(np.float32)
    (betas if which == "betas" else trans)[:2] = sc.TINY
    layer = _layer(monkeypatch, gpu_device, model, "tile", center_idx=12, max_batch=2)
    v, j = layer(*_dev(gpu_device, pose, betas, trans))
    r64 = smpl_ref64.forward(model, pose, betas, trans, 12)
    o32 = smpl_ref.smpl_forward(sc.oracle_model(model), pose, betas, trans, 12)
    for k, got, r, o in zip(("verts", "joints"), (v, j), r64, o32):
        ok, e_gpu, e_f32, bound = sc.check(got.cpu().numpy(), r, o)
        assert ok, f"{which} {k}: e_gpu {e_gpu:.3e}, bound {bound:.3e}"
    # ... and a chunk-wise decision would be centimetres away
    chunkwise = np.concatenate([smpl_ref64.forward(model, pose[s], betas[s], trans[s], 12)[0] for s in (slice(0, 2), slice(2, 4))])
    assert np.abs(chunkwise - r64[0]).max() > 1e-2


# ---- the handle ------------------------------------------------------------------------------------------------------

def test_centre_joint_out_of_range_is_refused(gpu_device, monkeypatch, body85):
    layer = _layer(monkeypatch, gpu_device, body85, "tile", center_idx=24)
    pose = torch.zeros((2, 72), device=gpu_device)
    with pytest.raises(_lib.PoseRiskHipError, match="center_idx"):
        layer(pose)
    layer.center_idx = 23
    v, j = layer(pose)
    assert float(j[:, 23].abs().max()) == 0.0 and bool(torch.isfinite(v).all())


@pytest.mark.parametrize("handle", list(sc.HANDLES))
def test_no_shape_coefficients(gpu_device, monkeypatch, handle):
    """NB = 0: th_betas None and the reference's placeholder torch.zeros(1) are the same call."""
    model = sc.make_model(85, 0, 4, "smpl", seed=78)
    layer = _layer(monkeypatch, gpu_device, model, handle)
    pose = np.random.default_rng(9).normal(0, 1.0, (19, 72)).astype(np.float32)
    p = _dev(gpu_device, pose)[0]
    a, b = layer(p, None), layer(p, torch.zeros(1))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    r64 = smpl_ref64.forward(model, pose)
    o32 = smpl_ref.smpl_forward(sc.oracle_model(model), pose)
    for k, got, r, o in zip(("verts", "joints"), a, r64, o32):
        ok, e_gpu, e_f32, bound = sc.check(got.cpu().numpy(), r, o)
        assert ok, f"{handle} {k}: e_gpu {e_gpu:.3e}, bound {bound:.3e}"


# ---- the library's own buffers between guards ------------------------------------------------------------------------------

@pytest.mark.parametrize("variant", list(sc.VARIANTS))
@pytest.mark.parametrize("mode", list(tf.MODES))
def test_sweep_under_the_internal_fence(gpu_device, monkeypatch, mode, variant):
    """The padded model rows (R), frame slots (Bs) and the [NNZ][V] ELL arrays are what these shapes stress: every case of the
    family with POSERISK_FENCE set -- guards intact, outputs finite and bit for bit the unfenced handle's."""
    for c in (c for c in sc.CASES if sc.variant(c) == variant):
        model, (pose, betas, trans), _, _ = sc.references(c.name)
        outs = {}
        for fenced in (None, mode):
            tf._set_mode(monkeypatch, fenced)
            layer = _layer(monkeypatch, gpu_device, model, c.handle, c.center_idx)
            names = tf.fence_names()
            assert ("smpl ell_w" in names and "smpl pm_T" in names) == (fenced is not None), sorted(names)
            outs[fenced] = _run(layer, gpu_device, pose, betas, trans)
            torch.cuda.synchronize()
            if fenced:
                tf.assert_fence_intact(f"{c.name} {mode}")
            del layer
        for k in OUTPUTS:
            assert bool(torch.isfinite(outs[mode][k]).all()) and torch.equal(outs[mode][k], outs[None][k]), \
                f"{c.name} {mode}: {k} differs from the unfenced handle's"
    tf.assert_fence_intact(f"{variant} {mode} after the handles were destroyed")
