"""Seeded synthetic stand-ins for the licensed assets the hot path needs.

The SPIN checkpoint, `smpl_mean_params.npz` and the SMPL `.pkl` files are licensed downloads
(reference README.md:36-37) and are absent here, so benchmarks and parity tests run on
random-initialised weights of the same architecture and a random SMPL model of the same sizes.
Everything is generated with NumPy PCG64 from fixed seeds and is reproducible without the
reference.
"""
import numpy as np

SMPL_PARENTS = (-1, 0, 0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 9, 9, 12, 13, 14, 16, 17, 18, 19, 20, 21)
RESNET_PLANES = (64, 128, 256, 512)
RESNET_BLOCKS = (3, 4, 6, 3)


def hmr_state_dict(seed=1):
    """SPIN-keyed state dict of HMR (float32 numpy arrays).

    He-normal convs (fan-out), BN gamma=1 beta=0 running_mean~N(0,0.1^2) running_var~U(0.5,1.5),
    PyTorch-default uniform FCs, Xavier(gain 0.01) decoders, init_pose = 6-D identity x24,
    init_shape = 0, init_cam = (0.9, 0, 0).
    """
    rng = np.random.Generator(np.random.PCG64(seed))
    sd = {}

    def conv(name, cout, cin, k):
        sd[name + ".weight"] = rng.normal(0.0, np.sqrt(2.0 / (k * k * cout)), (cout, cin, k, k)).astype(np.float32)

    def bn(name, c):
        sd[name + ".weight"] = np.ones(c, np.float32)
        sd[name + ".bias"] = np.zeros(c, np.float32)
        sd[name + ".running_mean"] = rng.normal(0.0, 0.1, c).astype(np.float32)
        sd[name + ".running_var"] = rng.uniform(0.5, 1.5, c).astype(np.float32)

    def linear(name, cout, cin, xavier_gain=None):
        if xavier_gain is None:
            b = 1.0 / np.sqrt(cin)
            sd[name + ".weight"] = rng.uniform(-b, b, (cout, cin)).astype(np.float32)
        else:
            b = xavier_gain * np.sqrt(6.0 / (cin + cout))
            sd[name + ".weight"] = rng.uniform(-b, b, (cout, cin)).astype(np.float32)
        bb = 1.0 / np.sqrt(cin)
        sd[name + ".bias"] = rng.uniform(-bb, bb, cout).astype(np.float32)

    conv("conv1", 64, 3, 7)
    bn("bn1", 64)
    inpl = 64
    for L, (pl, nb) in enumerate(zip(RESNET_PLANES, RESNET_BLOCKS), start=1):
        for b in range(nb):
            p = f"layer{L}.{b}"
            conv(p + ".conv1", pl, inpl, 1); bn(p + ".bn1", pl)
            conv(p + ".conv2", pl, pl, 3); bn(p + ".bn2", pl)
            conv(p + ".conv3", pl * 4, pl, 1); bn(p + ".bn3", pl * 4)
            if b == 0:
                conv(p + ".downsample.0", pl * 4, inpl, 1); bn(p + ".downsample.1", pl * 4)
            inpl = pl * 4
    linear("fc1", 1024, 2048 + 144 + 13)
    linear("fc2", 1024, 1024)
    linear("decpose", 144, 1024, xavier_gain=0.01)
    linear("decshape", 10, 1024, xavier_gain=0.01)
    linear("deccam", 3, 1024, xavier_gain=0.01)
    sd["init_pose"] = np.tile(np.array([1, 0, 0, 1, 0, 0], np.float32), 24).reshape(1, 144)
    sd["init_shape"] = np.zeros((1, 10), np.float32)
    sd["init_cam"] = np.array([[0.9, 0.0, 0.0]], np.float32)
    return sd


def crops(batch, seed=0):
    """f32[B,3,224,224] uniform [0,1): the un-normalised range CropDataset produces (Q1)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    return rng.random((batch, 3, 224, 224), dtype=np.float32)


def smpl_model(V=6890, seed=2, nnz=4, dense_weights=False, n_betas=10, model_betas=None):
    """Dict of the SMPL model constants with SMPL's shapes (J=24, 207 pose-blend columns).

    weights: each vertex is bound to `nnz` joints (like the real model's <=4) unless dense_weights;
    J_regressor: each joint regresses from 32 random vertices, rows sum to 1.
    """
    rng = np.random.Generator(np.random.PCG64(seed))
    J = 24
    v_template = (rng.normal(0.0, 0.3, (V, 3)) * np.array([0.6, 1.0, 0.3])).astype(np.float32)
    shapedirs = rng.normal(0.0, 0.01, (V, 3, n_betas)).astype(np.float32)
    posedirs = rng.normal(0.0, 0.005, (V, 3, (J - 1) * 9)).astype(np.float32)
    J_regressor = np.zeros((J, V), np.float32)
    for j in range(J):
        idx = rng.choice(V, size=min(32, V), replace=False)
        w = rng.random(idx.shape[0]).astype(np.float32) + 0.1
        J_regressor[j, idx] = w / w.sum()
    if dense_weights:
        weights = rng.random((V, J)).astype(np.float32)
    else:
        weights = np.zeros((V, J), np.float32)
        for v in range(V):
            idx = rng.choice(J, size=nnz, replace=False)
            weights[v, idx] = rng.random(nnz).astype(np.float32) + 0.05
    weights = (weights / weights.sum(axis=1, keepdims=True)).astype(np.float32)
    mb = np.zeros(n_betas, np.float32) if model_betas is None else np.asarray(model_betas, np.float32)
    return dict(v_template=v_template, shapedirs=shapedirs, posedirs=posedirs, J_regressor=J_regressor,
                weights=weights, parents=np.array(SMPL_PARENTS, np.int32), model_betas=mb)


def poses(n, seed=3, scale=0.3):
    """f32[n,72] axis-angle ~ N(0, scale^2)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    return rng.normal(0.0, scale, (n, 72)).astype(np.float32)


def betas(n, seed=4):
    rng = np.random.Generator(np.random.PCG64(seed))
    return rng.normal(0.0, 1.0, (n, 10)).astype(np.float32)


def rotmats(n, seed=5, scale=0.8):
    """f32[n,24,3,3] rotation matrices from random rot6d (Gram-Schmidt), like the regressor's output."""
    rng = np.random.Generator(np.random.PCG64(seed))
    x = rng.normal(0.0, scale, (n * 24, 3, 2)) + np.array([[1, 0], [0, 1], [0, 0]])
    a1, a2 = x[:, :, 0], x[:, :, 1]
    b1 = a1 / np.linalg.norm(a1, axis=1, keepdims=True)
    u = a2 - (b1 * a2).sum(1, keepdims=True) * b1
    b2 = u / np.linalg.norm(u, axis=1, keepdims=True)
    b3 = np.cross(b1, b2)
    return np.stack([b1, b2, b3], axis=-1).reshape(n, 24, 3, 3).astype(np.float32)


def genus0_mesh(V):
    """A closed genus-0 triangulation of exactly V >= 66 vertices on the unit sphere: the largest UV sphere (two poles,
    rings of 64) with at most V vertices, then each remaining vertex inserted into one face (+1 vertex, +2 faces), so
    F = 2 V - 4.  Synthetic SMPL models have no faces; this gives them a closed mesh with SMPL's counts (V = 6890 ->
    F = 13776).  Returns (vertices f32[V,3], faces int32[F,3])."""
    n_lon = 64
    n_lat = (V - 2) // n_lon
    th = np.pi * (np.arange(n_lat) + 1) / (n_lat + 1)
    ph = 2 * np.pi * np.arange(n_lon) / n_lon
    ring = np.stack([np.sin(th)[:, None] * np.cos(ph)[None], np.cos(th)[:, None] * np.ones_like(ph)[None],
                     np.sin(th)[:, None] * np.sin(ph)[None]], -1).reshape(-1, 3)
    nv = 2 + n_lat * n_lon
    verts = [np.array([0.0, 1.0, 0.0])] + list(ring) + [np.array([0.0, -1.0, 0.0])]
    rid = lambda i, j: 1 + i * n_lon + (j % n_lon)
    faces = [(0, rid(0, j + 1), rid(0, j)) for j in range(n_lon)]
    for i in range(n_lat - 1):
        for j in range(n_lon):
            a, b, c, d = rid(i, j), rid(i, j + 1), rid(i + 1, j), rid(i + 1, j + 1)
            faces += [(a, b, d), (a, d, c)]
    faces += [(nv - 1, rid(n_lat - 1, j), rid(n_lat - 1, j + 1)) for j in range(n_lon)]
    k = 0
    while nv < V:   # split face k into three around a new vertex at its (projected) centroid
        a, b, c = faces[k]
        m = verts[a] + verts[b] + verts[c]
        verts.append(m / np.linalg.norm(m))
        faces[k] = (a, b, nv)
        faces += [(b, c, nv), (c, a, nv)]
        nv += 1
        k += 2
    return np.array(verts, np.float32), np.array(faces, np.int32)


def closed_body(V=6890, seed=7):
    """A closed person-sized mesh with SMPL's counts (V = 6890, F = 13776): the genus-0 sphere stretched to a 1.7 m tall,
    0.5 m wide, 0.3 m deep body with a little surface noise, in SPIN's camera axes (y down), metres, centred on the
    origin.  Returns (vertices f32[V,3], faces int32[F,3])."""
    rng = np.random.Generator(np.random.PCG64(seed))
    v, f = genus0_mesh(V)
    v = v * np.array([0.25, 0.85, 0.15], np.float32) * (1 + 0.03 * rng.standard_normal((V, 1))).astype(np.float32)
    return v.astype(np.float32), f


def yolo_weights(seed=11):
    """The float body of a darknet YOLOv3 weight file, f32[62001757], whose outputs stay sane: the trained file is a download
    (multi_person_tracker fetches it), absent here.  Plain He weights let the 23 residual sums grow the activations to
    rms ~ 70 and |t| ~ 150 at the heads; these choices keep the heads near rms 2 with some person candidates:
    He-normal weights over the fan-out (as hmr_state_dict), with gain 0.3 on the 3x3 convolution of each residual block;
    BatchNorm gamma = 1, beta ~ N(0, 0.1^2), mean ~ N(0, 0.1^2), var ~ U(0.5, 1.5); head weights N(0, 0.6^2 / fan_in), head
    bias 0 for the box, -3 for the objectness, +3 for class 0 and -1 for the other classes (class 0 has to beat 79 others for
    a person candidate to exist: about a dozen a frame at 64 x 96 with conf_thres 0.1)."""
    from .detector import CONV, SHORTCUT, yolo_layers
    rng = np.random.Generator(np.random.PCG64(seed))
    layers = yolo_layers()
    parts = []
    for i, l in enumerate(layers):
        if l["type"] != CONV:
            continue
        fan_in, fan_out = l["cin"] * l["ksize"] ** 2, l["cout"] * l["ksize"] ** 2
        shape = (l["cout"], l["cin"], l["ksize"], l["ksize"])
        if l["bn"]:
            gain = 0.3 if i + 1 < len(layers) and layers[i + 1]["type"] == SHORTCUT else 1.0
            parts += [rng.normal(0.0, 0.1, l["cout"]), np.ones(l["cout"]), rng.normal(0.0, 0.1, l["cout"]), rng.uniform(0.5, 1.5, l["cout"])]
            parts.append(rng.standard_normal(shape, dtype=np.float32) * np.float32(gain * np.sqrt(2.0 / fan_out)))
        else:
            bias = np.zeros((3, 85))
            bias[:, 4], bias[:, 5], bias[:, 6:] = -3.0, 3.0, -1.0
            parts += [bias, rng.standard_normal(shape, dtype=np.float32) * np.float32(0.6 / np.sqrt(fan_in))]
    return np.concatenate([np.asarray(p, np.float32).ravel() for p in parts])


DEFAULT_INFO = {  # main/default_information.json
    "REBA": {"Legs_bilateral_weight_bearing/walking": 0, "Sitting": 0, "Load/Force Score": 0,
             "Arm_supported_leaning_L": 0, "Arm_supported_leaning_R": 0, "Coupling": 0, "Activity_Score": 0},
    "RULA": {"Arm_supported_leaning_L": 0, "Arm_supported_leaning_R": 0, "A_Muscle_use_L": 0,
             "A_Muscle_use_R": 0, "A_Load/Force_L": 0, "A_Load/Force_R": 0,
             "Legs_bilateral_weight_bearing": 0, "B_Muscle_use": 0, "B_Load/Force": 0},
}
EXAMPLE_INFO = {  # example/additional_information.json
    "REBA": dict(DEFAULT_INFO["REBA"], **{"Legs_bilateral_weight_bearing/walking": 1, "Sitting": 1}),
    "RULA": dict(DEFAULT_INFO["RULA"]),
}
