"""SMPL forward and get_joint_cam restated in float64, with nothing clever: the yardstick of tests/test_smpl_sweep_gpu.py.

Follows ``lib/smplpytorch/smplpytorch/pytorch/smpl_layer.py:65-158``, ``rodrigues_layer.py:13-52`` and
``lib/utils/coord_utils.py:7-21`` line by line, like oracle/smpl_ref.py, but every product and every sum is float64.
The inputs are the float32 arrays the kernels get, widened exactly.

What is NOT a matter of precision, and is therefore kept as the reference has it:
  * the norm is of (v + 1e-8), the division is by it but of v itself, and 1e-8 is the float32 constant (Q8);
  * the half-angle quaternion is normalised again before it is expanded;
  * "betas given?" and "trans given?" are ``torch.norm(x) == 0`` on float32 tensors: a float32 sum of float32 squares
    that is zero.  Values whose squares underflow (|x| <= 2^-75, about 2.6e-23) count as absent (Q9);
  * get_joint_cam overwrites the root row with (3.14, 0, 0), float32's 3.14.
"""
import numpy as np

F64 = np.float64
EPS_F32 = F64(np.float32(1e-8))
ROOT_F32 = F64(np.float32(3.14))


def batch_rodrigues(axisang):
    """rodrigues_layer.py:41-52 + quat2mat :13-38.  [N,3] -> f64[N,3,3]."""
    v = np.asarray(axisang, F64)
    norm = np.sqrt(((v + EPS_F32) ** 2).sum(axis=1))[:, None]
    axis = v / norm
    half = norm * 0.5
    q = np.concatenate([np.cos(half), np.sin(half) * axis], axis=1)
    q = q / np.sqrt((q * q).sum(axis=1))[:, None]
    w, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    w2, x2, y2, z2 = w * w, x * x, y * y, z * z
    wx, wy, wz, xy, xz, yz = w * x, w * y, w * z, x * y, x * z, y * z
    return np.stack([
        w2 + x2 - y2 - z2, 2 * xy - 2 * wz, 2 * wy + 2 * xz,
        2 * wz + 2 * xy, w2 - x2 + y2 - z2, 2 * yz - 2 * wx,
        2 * xz - 2 * wy, 2 * wx + 2 * yz, w2 - x2 - y2 + z2,
    ], axis=1).reshape(-1, 3, 3)


def all_zero_f32(x):
    """``x is None or torch.norm(x) == 0`` for a float32 tensor: the float32 sum of its float32 squares is zero."""
    if x is None:
        return True
    x = np.asarray(x, np.float32)
    return float((x * x).sum(dtype=np.float32)) == 0.0


def rest_joints(model, betas, B):
    """smpl_layer.py:85-95 -> (v_shaped f64[B or 1,V,3], joints f64[B,J,3], whether the model's betas were used)."""
    vt = np.asarray(model["v_template"], F64).reshape(-1, 3)
    V = vt.shape[0]
    sd = np.asarray(model["shapedirs"], F64)
    sd = sd.reshape(V, 3, sd.size // (3 * V))
    use_model = all_zero_f32(betas) or sd.shape[2] == 0
    mb = model.get("model_betas")
    b = (np.zeros((1, sd.shape[2])) if mb is None else np.asarray(mb, F64).reshape(1, -1)) if use_model \
        else np.asarray(betas, F64).reshape(B, -1)
    v_shaped = vt[None] + np.einsum("vcl,bl->bvc", sd, b)
    joints = np.einsum("jv,bvc->bjc", np.asarray(model["J_regressor"], F64), v_shaped)
    if use_model:
        joints = np.repeat(joints, B, axis=0)
    return v_shaped, joints, use_model


def chain(parents, R, joints):
    """smpl_layer.py:102-119: R f64[B,J,3,3], joints f64[B,J,3] -> G f64[B,J,4,4], for any topological tree."""
    B, J = R.shape[:2]
    G = np.zeros((B, J, 4, 4))
    G[:, :, 3, 3] = 1
    G[:, 0, :3, :3] = R[:, 0]
    G[:, 0, :3, 3] = joints[:, 0]
    for i in range(1, J):
        p = int(parents[i])
        assert 0 <= p < i, "not a topological tree"
        local = np.zeros((B, 4, 4))
        local[:, 3, 3] = 1
        local[:, :3, :3] = R[:, i]
        local[:, :3, 3] = joints[:, i] - joints[:, p]
        G[:, i] = G[:, p] @ local
    return G


def forward(model, pose, betas=None, trans=None, center_idx=None):
    """smpl_layer.py:65-158.  model: dict of v_template[V,3], shapedirs[V,3,NB], posedirs[V,3,207], J_regressor[J,V],
    weights[V,J], parents[J], optional model_betas[NB].  -> verts f64[B,V,3], joints f64[B,J,3]."""
    pose = np.asarray(pose, F64)
    B = pose.shape[0]
    parents = [int(p) for p in model["parents"]]
    J = len(parents)
    R = batch_rodrigues(pose.reshape(B * J, 3)).reshape(B, J, 3, 3)
    pose_map = (R[:, 1:] - np.eye(3)).reshape(B, (J - 1) * 9)                  # tensutils.py:41-48
    v_shaped, joints0, _ = rest_joints(model, betas, B)
    V = v_shaped.shape[1]
    v_posed = v_shaped + np.einsum("vcp,bp->bvc", np.asarray(model["posedirs"], F64).reshape(V, 3, -1), pose_map)
    G = chain(parents, R, joints0)
    A = G.copy()                                                               # smpl_layer.py:122-132
    A[:, :, :3, 3] = G[:, :, :3, 3] - np.einsum("bjrc,bjc->bjr", G[:, :, :3, :3], joints0)
    T = np.einsum("bjrc,vj->bvrc", A, np.asarray(model["weights"], F64))       # smpl_layer.py:134
    vh = np.concatenate([v_posed, np.ones((B, V, 1))], axis=2)
    verts = np.einsum("bvrc,bvc->bvr", T, vh)[:, :, :3]
    jtr = G[:, :, :3, 3].copy()
    if all_zero_f32(trans):                                                    # smpl_layer.py:147-155
        if center_idx is not None:
            c = jtr[:, center_idx][:, None]
            jtr, verts = jtr - c, verts - c
    else:
        t = np.asarray(trans, F64).reshape(B, 1, 3)
        jtr, verts = jtr + t, verts + t
    return verts, jtr


def joint_cam(model, axis_angle, center_idx=None, return_verts=False):
    """coord_utils.py:7-21 on [N,24,3]: root row (3.14, 0, 0), zero betas (so the model's own), millimetres, relative to
    the root.  The input is left alone.  return_verts: also the vertices of that forward, in metres, as the layer's
    joint_cam(return_verts=True) hands them out (not centred: the kernel's joint_cam entry has no centre)."""
    aa = np.array(axis_angle, F64).reshape(-1, 24, 3)
    aa[:, 0] = (ROOT_F32, 0.0, 0.0)
    verts, joints = forward(model, aa.reshape(-1, 72), np.zeros((1, 10), np.float32), None, None)
    if center_idx is not None:                       # the layer's own centring, which the root-relative step removes again
        joints = joints - joints[:, center_idx][:, None]
    j = joints * 1000.0
    jc = j - j[:, :1]
    return (jc, verts) if return_verts else jc
