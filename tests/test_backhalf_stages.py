"""Every stage behind the regressor, each from its own GPU input, at the batch sizes the pipeline launches it with: the outputs
of FramePipeline(..., with_verts=True) for whole batches (64 frames on the 64-frame handles, 256 frames on two lanes of the
256-frame handles, fp32 and bf16 encoder) and ragged ones (1, 7, 9, 217 frames) are taken apart stage by stage --

  regressor_finalize / rot6d   from the regressor tap's last state (tests/test_regressor_steps.py checks up to there)
  rotmat -> axis-angle -> Euler from the GPU's rotmat
  SMPL / joint_cam             from the GPU's axis-angle
  REBA / RULA                  from the GPU's Euler angles

-- every frame, joint and vertex, so that no stage's tolerance pays for the stage before it (end to end a bf16 encoder allows
5e-2 on everything behind it).  The inputs the pipeline never produces with synthetic weights (nearly parallel 6-D vectors,
rotations by almost pi and almost 0) go through ops.rot6d_to_rotmat and ops.pose_to_euler at the bottom."""
import numpy as np
import pytest
import torch

from conftest import measured
from oracle import coord_ref, hmr_ref, reba_ref, rodrigues_cv, rula_ref, smpl_ref
from poserisk_release_amd import ops, synth
from poserisk_release_amd.hmr import HMR
from poserisk_release_amd.pipeline import FramePipeline
from poserisk_release_amd.smpl_layer import SMPLLayer

pytestmark = pytest.mark.gpu

U = 2.0 ** -24     # float32 unit roundoff

# rot6d_one (csrc/frame_kernels.hip), counted in units of U, errors in the 2-norm, |a2| = beta, phi the angle between a1, a2:
#   n1 = sqrt(a1.a1): three products and two sums (3) halved by the root, plus the root's own rounding      2.5
#   b1 = a1 / n1: one division more                                                                          3.5 (relative)
#   d = b1.a2: 3.5 from b1 and 3 from the dot product, times beta                                            6.5 beta
#   u = a2 - d b1: d's error 6.5, b1's 3.5, the product's 1 and the difference's 1, times beta               12 beta
#   b2 = u / n2 with |u| = beta sin(phi): the direction of u errs by 12 / sin(phi) (normalising removes the part along u),
#        the normalisation itself by 3.5 as for b1                                                           12 / sin(phi) + 3.5
#   b3 = b1 x b2: b1's 3.5 + b2's + two products and a difference per component (3 sqrt 2 < 4.3)            12 / sin(phi) + 11.3
# Every entry of R is therefore within (12 / sin(phi) + 11.3) U <= 24 U / sin(phi) of the exact Gram-Schmidt (first order in
# U / sin(phi); fused multiply-adds only remove roundings).
C_ROT6D = 24.0

# name -> (encoder precision, frames, max_batch of the HMR and SMPL handles, lanes).  max_batch <= 128 skins with
# smpl_skin_tile, above with smpl_skin_rows; the handles are shared by the configurations of equal (precision, max_batch,
# lanes).  Ragged sizes: 8 frames per skinning block and 16 per regressor tile do not divide 1, 7, 9 or 217.
CONFIGS = {
    "fp32_B64": ("fp32", 64, 64, 1),
    "fp32_B256_lanes2": ("fp32", 256, 256, 2),
    "bf16_B256_lanes2": ("bf16", 256, 256, 2),
    "fp32_B1_tile": ("fp32", 1, 64, 1),
    "fp32_B7_tile": ("fp32", 7, 64, 1),
    "fp32_B9_tile": ("fp32", 9, 64, 1),
    "fp32_B1_rows": ("fp32", 1, 256, 2),
    "fp32_B7_rows": ("fp32", 7, 256, 2),
    "fp32_B9_rows": ("fp32", 9, 256, 2),
    "fp32_B217_rows": ("fp32", 217, 256, 2),
}
CROP_SEED = 33     # rot6d's condition below (99 % of a batch's joints with E <= 1e-5) holds for it; checked per batch

_SHARED = {}


def _shared(dev):
    if not _SHARED:
        _SHARED["sd"] = synth.hmr_state_dict(seed=1)
        sm = synth.smpl_model(V=6890, seed=2)
        _SHARED["sm"] = sm
        _SHARED["oracle_smpl"] = smpl_ref.SMPLModel(*(sm[k] for k in ("v_template", "shapedirs", "posedirs", "J_regressor", "weights")))
        _SHARED["pipes"] = {}
    return _SHARED


def _pipe(dev, precision, cap, lanes):
    sh = _shared(dev)
    key = (precision, cap, lanes)
    if key not in sh["pipes"]:
        m = HMR(max_batch=cap, precision=precision).to(dev)
        m.load_state_dict(sh["sd"])
        layer = SMPLLayer(sh["sm"], device=dev, max_batch=cap)
        sh["pipes"][key] = FramePipeline(m, layer, synth.EXAMPLE_INFO, with_verts=True, lanes=lanes)
    return sh["pipes"][key]


def _sin_phi(p6):
    """sin of the angle between a1 and a2 of every 6-D vector ([..., 6] float64, SPIN's view(-1, 3, 2)); 1 where one of them
    is the zero vector (nothing is orthogonalised then)."""
    a = p6.reshape(-1, 3, 2)
    a1, a2 = a[:, :, 0], a[:, :, 1]
    n = np.linalg.norm(a1, axis=1) * np.linalg.norm(a2, axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):      # directions first: norms of 1e-20 and 1e+15 stay well scaled
        s = np.linalg.norm(np.cross(a1 / np.linalg.norm(a1, axis=1, keepdims=True),
                                    a2 / np.linalg.norm(a2, axis=1, keepdims=True)), axis=1)
    return np.where(n > 0, s, 1.0)


def _rot6d_ref(p6):
    """hmr_ref.rot6d_to_rotmat in float64 (the same max(norm, 1e-12)) -> ([n, 3, 3], E [n] per joint)."""
    ref = hmr_ref.rot6d_to_rotmat(torch.from_numpy(p6.astype(np.float64))).numpy()
    return ref, C_ROT6D * U / _sin_phi(p6.astype(np.float64))


def _check_rotmat_to_euler(tag, rotmat, aa, eul):
    """test_pose_to_euler_matches_golden's criteria on every joint: the float32 axis-angle within one float32 ulp of the
    vector's largest component of oracle.rodrigues_cv in double; the Euler angles through the oracle's Euler stage applied to
    OUR axis-angle within 1e-5 degrees, 99.9 % within 1e-9."""
    R = rotmat.reshape(-1, 3, 3).astype(np.float64)
    ref = np.stack([rodrigues_cv.rotmat_to_rotvec(m) for m in R]).reshape(aa.shape)
    big = np.abs(ref).max(axis=-1, keepdims=True).astype(np.float32)
    ulp = np.spacing(np.maximum(big, np.float32(1e-30))).astype(np.float64)
    off = np.abs(aa.astype(np.float64) - ref) / ulp
    measured(f"{tag}: axis-angle vs rodrigues_cv in double (float32 ulps of the largest component)", off.max(), 1.0, "ulp")
    assert off.max() <= 1.0, off.max()
    theta = np.linalg.norm(ref, axis=-1)
    want = np.stack([coord_ref.axis_angle_to_euler_angle(f) for f in aa])
    d = np.abs(eul - want)
    d = np.minimum(d, 360 - d)
    measured(f"{tag}: Euler vs the oracle's Euler stage on our axis-angle", d.max(), 1e-5, "deg")
    assert d.max() < 1e-5 and np.mean(d < 1e-9) > 0.999, (d.max(), np.mean(d < 1e-9))
    return float(theta.min()), float(theta.max())


def _check_lane(tag, dev, out, x):
    sh = _shared(dev)
    B = x.shape[0]
    got = {k: v.clone() for k, v in out.items()}
    hmr = out.lane.hmr
    with torch.no_grad():
        rot_f, betas_f, cam_f, xf, p6 = hmr(x, return_features=True)
        state = hmr.regress_until(xf, 10)
    # ---- regressor_finalize: copies of the state's columns; the pipeline's rotmat is the forward's
    assert torch.equal(p6, state[:, :144]) and torch.equal(got["betas"], state[:, 144:154])
    assert torch.equal(got["cam"], state[:, 154:157])
    assert torch.equal(got["betas"], betas_f) and torch.equal(got["cam"], cam_f) and torch.equal(got["rotmat"], rot_f)
    # ---- rot6d against Gram-Schmidt in float64 on the GPU's pose6d
    rotmat = got["rotmat"].cpu().numpy()
    ref, E = _rot6d_ref(p6.cpu().numpy())
    share = float(np.mean(E <= 1e-5))
    measured(f"{tag}: share of joints with the rot6d bound <= 1e-5", share)
    measured(f"{tag}: smallest sin(phi)", (C_ROT6D * U / E).min())
    assert share >= 0.99, (share, "choose other crop seeds")
    err = np.abs(rotmat.reshape(-1, 3, 3).astype(np.float64) - ref)
    r = (err / E[:, None, None]).max()
    measured(f"{tag}: rotmat vs fp64 Gram-Schmidt, max error / E", r, 1.0)
    measured(f"{tag}: rotmat vs fp64 Gram-Schmidt, max error", err.max())
    assert r <= 1.0, r
    # ---- rotmat -> axis-angle -> Euler: the stand-alone entry gives the pipeline's bits, root rows included
    aa_full, eul2, st2 = ops.pose_to_euler(got["rotmat"])
    assert torch.equal(aa_full[:, 1:], got["axis_angle"][:, 1:]) and torch.equal(eul2, got["euler"])
    assert int(got["status"].abs().sum()) == 0 and int(st2.abs().sum()) == 0
    aa = aa_full.cpu().numpy()
    eul = got["euler"].cpu().numpy()
    tmin, tmax = _check_rotmat_to_euler(tag, rotmat, aa, eul)
    measured(f"{tag}: smallest rotation angle", tmin, unit="rad")
    measured(f"{tag}: largest rotation angle", tmax, unit="rad")
    # ---- SMPL: the axis-angle as pr_smpl_joint_cam received it (root rows restored; the oracle overwrites them itself)
    assert np.all(got["axis_angle"][:, 0].cpu().numpy() == np.array([3.14, 0, 0], np.float32))
    om = sh["oracle_smpl"]
    pose = aa.copy()
    want_jc = coord_ref.get_joint_cam(pose, lambda p, b: smpl_ref.smpl_forward(om, p, b))
    np.testing.assert_array_equal(pose, got["axis_angle"].cpu().numpy())     # the same in-place overwrite
    e_jc = np.abs(got["joint_cam"].cpu().numpy().astype(np.float64) - want_jc).max()
    measured(f"{tag}: joint_cam vs oracle.smpl_ref from our axis-angle", e_jc, 1e-2, "mm")
    assert e_jc <= 1e-2, e_jc
    verts = got["verts"].cpu().numpy()
    e_v = 0.0
    for f0 in range(0, B, 16):
        want_v, _ = smpl_ref.smpl_forward(om, pose[f0:f0 + 16].reshape(-1, 72), np.zeros((min(16, B - f0), 10), np.float32))
        e_v = max(e_v, float(np.abs(verts[f0:f0 + 16].astype(np.float64) - want_v).max()))
    measured(f"{tag}: verts vs oracle.smpl_ref from our axis-angle", e_v, 1e-5, "m")
    assert e_v <= 1e-5, e_v
    # ---- scores from our Euler angles: exact
    info = synth.EXAMPLE_INFO
    np.testing.assert_array_equal(got["reba"].cpu().numpy(), reba_ref.reba_packed(eul, info["REBA"]))
    np.testing.assert_array_equal(got["rula"].cpu().numpy(), rula_ref.rula_packed(eul, info["RULA"]))


@pytest.mark.parametrize("name", list(CONFIGS))
def test_stages_behind_the_regressor(gpu_device, name):
    precision, B, cap, lanes = CONFIGS[name]
    pipe = _pipe(gpu_device, precision, cap, lanes)
    x = torch.from_numpy(synth.crops(B, seed=CROP_SEED)).to(gpu_device)
    xs = [x] + [x.flip(0).contiguous() for _ in range(1, lanes)]      # the other lane: the frames in reverse order
    outs = [pipe(xi) for xi in xs]
    for o in outs:
        FramePipeline.wait(o)
    pipe.synchronize()
    assert len({id(o.lane) for o in outs}) == lanes
    for i, (o, xi) in enumerate(zip(outs, xs)):
        _check_lane(f"{name} lane {i}" if lanes > 1 else name, gpu_device, o, xi)


# ---- inputs the pipeline never produces ----------------------------------------------------------------------------------
N_SYN = 256          # frames of 24 joints


def _unit(rng, n):
    v = rng.standard_normal((n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _perp(rng, a):
    v = _unit(rng, a.shape[0])
    v -= (v * a).sum(1, keepdims=True) * a
    return v / np.linalg.norm(v, axis=1, keepdims=True)


ROT6D_CASES = [f"sin {s:g}" for s in (1e-1, 1e-2, 1e-3, 1e-4, 1e-5, 1e-6)] + \
              ["a2 = 0", "a1 = 0", "|a1| 1e-20", "|a2| 1e-20", "both 1e-20", "|a1| 1e+15", "|a2| 1e+15", "benign"]


def test_rot6d_degenerate_inputs(gpu_device):
    """Nearly parallel, vanishing, tiny and huge 6-D vectors against hmr_ref.rot6d_to_rotmat in float64.  The bound is the
    pipeline's, C_ROT6D U / sin(phi): it grows as the two vectors align -- at sin(phi) = 1e-6 it is 1.4 and says nothing, at
    1e-3 it is 1.4e-3 -- because the orthogonalised a2 is a difference of nearly equal float32 vectors."""
    rng = np.random.default_rng(5)
    n = N_SYN * 24
    case = np.arange(n) % len(ROT6D_CASES)
    a1 = _unit(rng, n)
    sin = rng.uniform(0.3, 1.0, n)
    for i, v in enumerate((1e-1, 1e-2, 1e-3, 1e-4, 1e-5, 1e-6)):
        sin[case == i] = v
    a2 = np.sqrt(1 - sin ** 2)[:, None] * a1 + sin[:, None] * _perp(rng, a1)
    s1, s2 = rng.uniform(0.5, 2.0, (n, 1)), rng.uniform(0.5, 2.0, (n, 1))
    for label, (f1, f2) in {"a2 = 0": (None, 0.0), "a1 = 0": (0.0, None), "|a1| 1e-20": (1e-20, None),
                            "|a2| 1e-20": (None, 1e-20), "both 1e-20": (1e-20, 1e-20), "|a1| 1e+15": (1e15, None),
                            "|a2| 1e+15": (None, 1e15)}.items():
        m = case == ROT6D_CASES.index(label)
        if f1 is not None:
            s1[m] = f1
        if f2 is not None:
            s2[m] = f2
    p6 = np.stack([a1 * s1, a2 * s2], axis=2).reshape(N_SYN, 144).astype(np.float32)      # view(-1, 3, 2): a1, a2 interleaved
    got = ops.rot6d_to_rotmat(torch.from_numpy(p6).to(gpu_device)).cpu().numpy().reshape(-1, 3, 3).astype(np.float64)
    ref, E = _rot6d_ref(p6)
    assert np.isfinite(got).all()
    zero = ref == 0
    assert zero.sum() >= 2 * 6 * (n // len(ROT6D_CASES)) and (got[zero] == 0).all()     # b2, b3 of a2 = 0; b1, b3 of a1 = 0
    r = np.abs(got - ref) / E[:, None, None]
    for i, label in enumerate(ROT6D_CASES):
        m = case == i
        measured(f"rot6d synthetic, {label}: max error / E", r[m].max(), 1.0)
        measured(f"rot6d synthetic, {label}: max error", np.abs(got - ref)[m].max())
    assert r.max() <= 1.0, r.max()


def _rotmats(axis, theta):
    """Rodrigues' formula in float64: [n, 3, 3]."""
    K = np.zeros((axis.shape[0], 3, 3))
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 0] = -axis[:, 2], axis[:, 1], axis[:, 2]
    K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -axis[:, 0], -axis[:, 1], axis[:, 0]
    s, c = np.sin(theta)[:, None, None], np.cos(theta)[:, None, None]
    return c * np.eye(3) + (1 - c) * axis[:, :, None] * axis[:, None, :] + s * K


def _cv_branch(R):
    """OpenCV's branch variable of one matrix (float64 [3, 3]) and what its OTHER small-angle branch would return: s = |skew
    part| / 2 of the orthonormalised matrix decides between the zero vector (s < 1e-5, cos > 0) and theta / (2 s) times the
    skew part -> (s, that vector)."""
    U, _, Vt = np.linalg.svd(R)
    Q = U @ Vt
    r = np.array([Q[2, 1] - Q[1, 2], Q[0, 2] - Q[2, 0], Q[1, 0] - Q[0, 1]])
    sn = np.sqrt((r * r).sum() * 0.25)
    theta = np.arccos(min(1.0, max(-1.0, (np.trace(Q) - 1.0) * 0.5)))
    return sn, r * (theta / (2.0 * sn))


THETAS = [np.pi - 10.0 ** -k for k in range(2, 9)] + [10.0 ** -k for k in range(3, 10)]


@pytest.mark.parametrize("source", ["rounded", "rot6d"])
def test_rodrigues_near_pi_and_near_zero(gpu_device, source):
    """Rotations by pi - {1e-2 .. 1e-8} and by {1e-3 .. 1e-9} about random axes against oracle.rodrigues_cv in double:
    `rounded` = the float32 rounding of the float64 matrix, `rot6d` = the GPU's own rot6d of its first two columns (nearly,
    not exactly, orthonormal: what the kernel's polar-factor iteration is for).  Criterion: the axis-angle vector within one
    float32 ulp of its largest component, plus what the oracle itself cannot know: OpenCV takes theta = acos((tr R - 1) / 2) of
    the orthonormalised matrix in double, and acos amplifies an error of its argument by 1 / sin(theta).  The two
    orthonormalisations (an SVD there, a Newton iteration here) agree to a few double ulps per entry; with 4 ulps (2^-52) on
    each side's argument that is 8 * 2^-52 / sin(theta) -- 1.8e-10 at theta = 1e-5, twenty float32 ulps of such a vector,
    nothing next to an ulp from theta = 1e-3 on.  OpenCV's result also JUMPS where the sine it measures crosses 1e-5 (below:
    the zero vector, above: theta times the axis), and the rotations by exactly 1e-5 sit on that jump: sin(1e-5) is 1.7e-11
    below 1e-5 relatively, the float32 rounding of the matrix moves it by ~3e-8 either way, and the two orthonormalisations
    see it ~1e-11 apart (1e-16 absolute on entries of 1e-5).  A joint whose sine is within 1e-9 of the threshold may
    therefore take either branch's value (one of 439 such joints did on the MI355X: the oracle returned zero, the kernel
    1e-5 times the axis); how many did is reported.  (Without the term the rotations by 1e-4 and 1e-5 miss one ulp: measured 1.4
    and 35 ulps, 1e-12 and 3e-11 absolute, the rebuilt matrices within 2e-11.)  Within 1e-5 of pi the sign of the vector is a convention of OpenCV's branch (v and
    -v are the same rotation there to that order), so a joint that misses the vector criterion there passes if the rotation
    matrix rebuilt from it is within 2^-22 of the one rebuilt from the oracle's; how many needed that is reported."""
    rng = np.random.default_rng(9)
    n = N_SYN * 24
    theta = np.array(THETAS)[np.arange(n) % len(THETAS)]
    R = _rotmats(_unit(rng, n), theta)
    if source == "rounded":
        R32 = torch.from_numpy(R.astype(np.float32).reshape(N_SYN, 24, 3, 3)).to(gpu_device)
    else:
        p6 = R[:, :, :2].reshape(N_SYN, 144).astype(np.float32)          # [3, 2] per joint: columns b1, b2 interleaved
        R32 = ops.rot6d_to_rotmat(torch.from_numpy(p6).to(gpu_device))
        dev = np.abs(R32.cpu().numpy().reshape(-1, 3, 3).astype(np.float64) - R).max()
        measured("rodrigues synthetic: the GPU's rot6d of two columns vs the float64 matrix", dev, 1e-6)
        assert dev <= 1e-6
    aa, _, _ = ops.pose_to_euler(R32)
    aa = aa.cpu().numpy().reshape(-1, 3).astype(np.float64)
    Rin = R32.cpu().numpy().reshape(-1, 3, 3).astype(np.float64)
    ref = np.stack([rodrigues_cv.rotmat_to_rotvec(m) for m in Rin])
    ulp = np.spacing(np.maximum(np.abs(ref).max(axis=1).astype(np.float32), np.float32(1e-30))).astype(np.float64)
    theta_ref = np.linalg.norm(ref, axis=1)
    with np.errstate(divide="ignore"):
        acos_term = np.where(theta_ref > 0, 8 * 2.0 ** -52 / np.abs(np.sin(theta_ref)), 0.0)
    off = np.abs(aa - ref).max(axis=1) / (ulp + acos_term)
    vec_ok = off <= 1.0
    near_pi = np.abs(theta_ref - np.pi) <= 1e-5
    dR = np.array([np.abs(rodrigues_cv.rotvec_to_rotmat(a) - rodrigues_cv.rotvec_to_rotmat(b)).max() for a, b in zip(aa, ref)])
    mat_ok = dR <= 2.0 ** -22
    needed = int((~vec_ok & near_pi).sum())
    measured(f"rodrigues synthetic ({source}): joints within 1e-5 of pi compared through the rebuilt matrix", needed)
    measured(f"rodrigues synthetic ({source}): axis-angle / (ulp + acos term) where compared as a vector", off[vec_ok].max(), 1.0)
    measured(f"rodrigues synthetic ({source}): rebuilt rotation matrix, max difference near pi", dR[near_pi].max(), 2.0 ** -22)
    on_jump = 0
    for i in np.flatnonzero(~vec_ok & (theta == 1e-5)):
        sn, other = _cv_branch(Rin[i])
        if abs(sn / 1e-5 - 1.0) < 1e-9:
            alt = other if not ref[i].any() else np.zeros(3)
            tol = np.spacing(np.float32(max(np.abs(alt).max(), 1e-30))).astype(np.float64) + 8 * 2.0 ** -52 / 1e-5
            if np.abs(aa[i] - alt).max() <= tol:
                vec_ok[i] = True
                on_jump += 1
    measured(f"rodrigues synthetic ({source}): joints on the 1e-5 jump that took the other branch", on_jump)
    bad = ~(vec_ok | (near_pi & mat_ok))
    assert not bad.any(), (int(bad.sum()), theta[bad][:5], off[bad][:5], dR[bad][:5])
    assert mat_ok[near_pi].all(), float(dR[near_pi].max())
    # rotations below OpenCV's 1e-5 threshold on sin(theta) come out as the zero vector, in both
    tiny = theta < 5e-6
    assert (ref[tiny] == 0).all() and (aa[tiny] == 0).all()
