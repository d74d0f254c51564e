"""Models, inputs, cases and the comparison of the SMPL sweep (tests/test_smpl_sweep_*.py, tests/golden/make_golden.py).

The models are made here, not by poserisk_release_amd.synth (whose streams the older goldens depend on): any vertex count,
0 to 16 shape coefficients, a per-vertex number of skinning weights drawn from 1..nnz_max with the last vertex at the
maximum and (where nnz_max > 1 and there are three vertices) the middle one with no weight at all, and any topological
kinematic tree.

The case list is not a full product.  Every kernel instantiation behind pr_smpl_forward's dispatch meets every vertex-count
class once; the other axes are dealt least-used-first, and a few cases are added by hand for what the deal cannot aim at
(the chunk edge with a translation, the edge poses on the dense kernels).  tests/test_smpl_sweep_cpu.py holds the list
to its coverage.

The comparison: `e_f32` is what a float32 restatement in another order (oracle.smpl_ref) is away from float64
(tests/smpl_ref64.py) on the very same case and output, and a kernel may be twice that plus one float32 spacing at the
output's largest magnitude away.  The bound never looks at the kernel's own figures.
"""
import collections
import functools
import math

import numpy as np

import smpl_ref64
from oracle import smpl_ref

F32 = np.float32
J = 24
NP = (J - 1) * 9

V_CLASSES = (1, 21, 22, 84, 85, 169, 673)     # tile edges (21 / 84 vertices), first vertex behind a group of 8 tiles
NNZ_VALUES = (1, 3, 4, 5, 8, 9, 24)
NB_VALUES = (0, 1, 9, 10, 11, 16)
TREES = ("smpl", "chain", "star", "random")
CENTERS = (None, 0, 12, 23)
TRANS = ("absent", "zero", "nonzero")
POSES = ("n03", "n1", "n3", "twopi", "edges")
MIN_VALUES = 2000                              # output values per case, so that a maximum is a stable statistic
# (max_batch, POSERISK_SMPL_TILE): the register-tiled kernel where it applies, the wave-split one, the rows kernels
HANDLES = {"tile": (17, "1"), "split": (17, "0"), "rows": (129, None)}
VARIANTS = ("tile<4>", "split<4>", "split<8>", "split<24>", "rows<4>", "rows<8>", "rows<24>")

# rodrigues.npz's edge vectors: zero, below the 1e-8 of the norm, tiny, 3.14 and float32's pi
EDGE_VECTORS = np.array([[0, 0, 0], [1e-9, 1e-9, 1e-9], [1e-6, 0, 0], [0, -1e-7, 2e-7], [3.14, 0, 0], [0, 3.1415927, 0]], F32)

Case = collections.namedtuple("Case", "name V nnz_max NB handle B tree center_idx trans pose seed")


def batch_sizes(max_batch):
    return (1, 15, 16, 17, max_batch, max_batch + 1, 2 * max_batch + 3)


def variant(c):
    """The skinning kernel pr_smpl_forward launches for the case (csrc/smpl.hip, smpl_run_chunk)."""
    max_batch, tile = HANDLES[c.handle]
    t = 4 if c.nnz_max <= 4 else 8 if c.nnz_max <= 8 else 24
    if max_batch > 128:
        return f"rows<{t}>"
    if tile == "1" and c.nnz_max <= 4 and c.NB <= 10:
        return "tile<4>"
    return f"split<{t}>"


def tile_eligible(c):
    return HANDLES[c.handle][0] <= 128 and c.nnz_max <= 4 and c.NB <= 10


def parents_of(tree, seed=0):
    if tree == "smpl":
        return np.array(smpl_ref.SMPL_PARENTS, np.int32)
    if tree == "chain":                                   # depth 23: one joint per level
        return np.arange(-1, J - 1, dtype=np.int32)
    if tree == "star":                                    # depth 1: every joint hangs on the root
        return np.array([-1] + [0] * (J - 1), np.int32)
    rng = np.random.Generator(np.random.PCG64(1000 + seed))
    return np.array([-1] + [int(rng.integers(0, i)) for i in range(1, J)], np.int32)


def make_model(V, NB, nnz_max, tree="smpl", seed=0, model_betas=False):
    rng = np.random.Generator(np.random.PCG64(seed))
    v_template = (rng.normal(0.0, 0.3, (V, 3)) * np.array([0.6, 1.0, 0.3])).astype(F32)
    shapedirs = rng.normal(0.0, 0.01, (V, 3, NB)).astype(F32)
    posedirs = rng.normal(0.0, 0.005, (V, 3, NP)).astype(F32)
    J_regressor = np.zeros((J, V), F32)
    for j in range(J):
        idx = rng.choice(V, size=min(32, V), replace=False)
        w = rng.random(idx.shape[0]).astype(F32) + F32(0.1)
        J_regressor[j, idx] = w / w.sum()
    count = rng.integers(1, nnz_max + 1, V)
    count[V - 1] = nnz_max
    if nnz_max > 1 and V >= 3:
        count[V // 2] = 0
    weights = np.zeros((V, J), F32)
    for v in range(V):
        if count[v]:
            idx = rng.choice(J, size=int(count[v]), replace=False)
            w = rng.random(int(count[v])).astype(F32) + F32(0.05)
            weights[v, idx] = w / w.sum()
    mb = np.linspace(-0.5, 0.5, NB).astype(F32) if model_betas else np.zeros(NB, F32)
    return dict(v_template=v_template, shapedirs=shapedirs, posedirs=posedirs, J_regressor=J_regressor, weights=weights,
                parents=parents_of(tree, seed), model_betas=mb)


def oracle_model(m):
    return smpl_ref.SMPLModel(m["v_template"], m["shapedirs"], m["posedirs"], m["J_regressor"], m["weights"],
                              parents=m["parents"], model_betas=m["model_betas"])


def make_pose(kind, B, seed):
    rng = np.random.Generator(np.random.PCG64(2000 + seed))
    scale = {"n03": 0.3, "n1": 1.0, "n2": 2.0, "n3": 3.0, "twopi": 1.0, "edges": 0.3}[kind]
    pose = rng.normal(0.0, scale, (B, J, 3)).astype(F32)
    if kind == "twopi":                                   # frame 0: every joint exactly 2 pi or 4 pi about one axis
        pose[0] = 0
        for j in range(J):
            pose[0, j, j % 3] = F32((2 + 2 * (j & 1)) * math.pi) * (-1 if j & 2 else 1)
    if kind == "edges":
        pose[0] = EDGE_VECTORS[(np.arange(J) + 1) % len(EDGE_VECTORS)]
    return pose.reshape(B, J * 3)


def make_inputs(c):
    """-> pose f32[B,72], betas f32[B,NB] | None (NB = 0), trans f32[B,3] | None; different in every frame."""
    rng = np.random.Generator(np.random.PCG64(3000 + c.seed))
    pose = make_pose(c.pose, c.B, c.seed)
    betas = rng.normal(0.0, 1.0, (c.B, c.NB)).astype(F32) if c.NB else None
    t = (rng.normal(0.0, 0.3, (c.B, 3))).astype(F32)
    trans = {"absent": None, "zero": np.zeros((c.B, 3), F32), "nonzero": t}[c.trans]
    return pose, betas, trans


def case_model(c):
    return make_model(c.V, c.NB, c.nnz_max, c.tree, seed=c.seed)


def _nnz_of(v):
    return {"4": (1, 3, 4), "8": (5, 8), "24": (9, 24)}[v[v.index("<") + 1:-1]]


def _build_cases():
    used = collections.Counter()

    def deal(axis, values):                               # the least-used value so far, in the axis' own order on a tie
        v = min(values, key=lambda x: (used[axis, x], values.index(x)))
        used[axis, v] += 1
        return v

    def batch(handle, V):
        sizes = batch_sizes(HANDLES[handle][0])
        ok = [b for b in sizes if b * V * 3 >= MIN_VALUES]
        return deal(("B", handle), ok) if ok else -(-MIN_VALUES // (V * 3))       # tiny V: B raised past the list

    cases = []

    def add(V, nnz, NB, handle, B=None, tree=None, ct=None, pose=None):
        center, trans = ct if ct is not None else deal("ct", [(a, b) for a in CENTERS for b in TRANS])
        B = B if B is not None else batch(handle, V)
        # (a lone frame of whole turns is the rest pose: every joint's transform the same, a wrong weight order invisible
        # -- tests/test_smpl_sweep_checker.py found that --, so the two special frames come with random ones behind them)
        c = Case("", V, nnz, NB, handle, B, tree or deal("tree", TREES), center, trans,
                 pose or deal("pose", POSES if B > 1 else POSES[:3]), len(cases))
        cases.append(c._replace(name=f"{len(cases):02d}-{variant(c).replace('<', '').replace('>', '')}-V{c.V}-k{c.nnz_max}-nb{c.NB}-B{c.B}-{c.tree}-"
                                     f"c{c.center_idx}-t{c.trans}-{c.pose}"))

    for var in VARIANTS:
        for i, V in enumerate(V_CLASSES):
            nnz = deal(("nnz", var[-3:]), _nnz_of(var))
            if var == "tile<4>":
                add(V, nnz, deal("NB tile", (0, 1, 9, 10)), "tile")
            elif var == "split<4>" and i % 3 == 1:        # the tile kernel switched on, but more than 10 coefficients
                add(V, nnz, deal("NB fallback", (11, 16)), "tile")
            else:
                add(V, nnz, deal("NB", NB_VALUES), "rows" if var.startswith("rows") else "split")
    # by hand: a translation across the chunk edge, a given-but-zero one with a centre, the edge poses on the dense kernels
    for h in HANDLES:
        mb = HANDLES[h][0]
        add(85, 4, 10, h, B=2 * mb + 3, tree="smpl", ct=(None, "nonzero"), pose="n1")
        add(169, 3, 9, h, B=mb + 1, tree="random", ct=(12, "zero"), pose="n3")
    add(84, 8, 10, "split", B=18, tree="chain", ct=(23, "absent"), pose="twopi")
    add(84, 5, 16, "rows", B=130, tree="chain", ct=(0, "nonzero"), pose="twopi")
    add(22, 24, 16, "split", B=37, tree="star", ct=(12, "absent"), pose="edges")
    add(22, 9, 11, "rows", B=261, tree="star", ct=(23, "zero"), pose="edges")
    add(22, 4, 0, "tile", B=37, tree="smpl", ct=(0, "absent"), pose="edges")
    return tuple(cases)


CASES = _build_cases()
BY_NAME = {c.name: c for c in CASES}


# ---- the fixtures of tests/golden/smpl_sweep.npz: what the reference's own SMPL_Layer gives (make_golden.py) ---------

def _fixture_specs():
    f = {}
    base = dict(V=22, NB=10, nnz_max=4, tree="smpl", model_betas=False, center_idx=None, trans="absent", betas="rand", pose="n03")
    for c in (0, 12, 23):
        for t in TRANS:
            f[f"centre{c}_trans_{t}"] = dict(base, center_idx=c, trans=t)
    f["pose_scale_2"] = dict(base, pose="n2")
    f["two_pi_four_pi"] = dict(base, pose="twopi")
    tiny = dict(base, model_betas=True, center_idx=12)
    f["tiny_betas_tiny_trans"] = dict(tiny, betas="tiny", trans="tiny")
    f["tiny_betas"] = dict(tiny, betas="tiny", trans="nonzero")
    f["tiny_trans"] = dict(tiny, betas="rand", trans="tiny")
    f["tree_chain"] = dict(base, tree="chain", pose="n1")
    f["tree_star"] = dict(base, tree="star", pose="n1")
    for k in (1, 5, 9):
        f[f"weights_{k}"] = dict(base, nnz_max=k)
    return f


FIXTURES = _fixture_specs()
FIXTURE_FRAMES = 3
TINY = 1e-23                                   # its float32 square underflows: torch.norm(x) == 0 holds for such a tensor


def fixture_model(name):
    s = FIXTURES[name]
    return make_model(s["V"], s["NB"], s["nnz_max"], s["tree"], seed=500 + list(FIXTURES).index(name), model_betas=s["model_betas"])


def fixture_inputs(name):
    """-> pose, betas, trans (None: not passed to the layer) of the fixture, as make_golden.py stores them."""
    s, B = FIXTURES[name], FIXTURE_FRAMES
    seed = 600 + list(FIXTURES).index(name)
    rng = np.random.Generator(np.random.PCG64(seed))
    betas = np.full((B, s["NB"]), TINY, F32) if s["betas"] == "tiny" else rng.normal(0.0, 1.0, (B, s["NB"])).astype(F32)
    t = rng.normal(0.0, 0.3, (B, 3)).astype(F32)
    trans = {"absent": None, "zero": np.zeros((B, 3), F32), "nonzero": t, "tiny": np.full((B, 3), TINY, F32)}[s["trans"]]
    return make_pose(s["pose"], B, seed), betas, trans


# ---- references -----------------------------------------------------------------------------------------------------

def oracle_joint_cam(om, pose):
    """get_joint_cam in float32 with oracle.smpl_ref (batched; oracle.coord_ref's loop frame by frame does the same
    arithmetic) -> joint_cam f32[B,24,3] in millimetres, the vertices of that forward."""
    aa = np.array(pose, F32).reshape(-1, J, 3)
    aa[:, 0] = np.array([3.14, 0, 0], F32)
    v, j = smpl_ref.smpl_forward(om, aa.reshape(-1, J * 3), np.zeros((1, 10), F32))
    j = j * F32(1000)
    return j - j[:, :1], v


@functools.lru_cache(maxsize=None)
def references(name):
    """-> (model, inputs, ref64 {output: f64}, oracle {output: f32}) of the case; computed once, never written to."""
    c = BY_NAME[name]
    m = case_model(c)
    pose, betas, trans = make_inputs(c)
    om = oracle_model(m)
    r64, o32 = {}, {}
    r64["verts"], r64["joints"] = smpl_ref64.forward(m, pose, betas, trans, c.center_idx)
    o32["verts"], o32["joints"] = smpl_ref.smpl_forward(om, pose, betas, trans, c.center_idx)
    r64["joint_cam"], r64["joint_cam verts"] = smpl_ref64.joint_cam(m, pose.reshape(-1, J, 3), return_verts=True)
    o32["joint_cam"], o32["joint_cam verts"] = oracle_joint_cam(om, pose)
    for d in (r64, o32):
        for a in d.values():
            a.setflags(write=False)
    return m, (pose, betas, trans), r64, o32


def bound(ref64, oracle32):
    """-> (e_f32, the most a kernel may be away from ref64): twice the float32 oracle's own error -- the margin for another
    summation order and the device's sinf / cosf -- plus one float32 spacing at the output's largest magnitude (the
    oracle's joint error is exactly 0 where V = 1)."""
    e_f32 = float(np.abs(np.asarray(oracle32, np.float64) - ref64).max())
    return e_f32, 2.0 * e_f32 + float(np.spacing(F32(np.abs(ref64).max())))


def check(got, ref64, oracle32):
    """-> (ok, e_gpu, e_f32, bound).  A NaN anywhere fails."""
    e_f32, b = bound(ref64, oracle32)
    got = np.asarray(got, np.float64)
    e = float(np.abs(got - ref64).max()) if got.shape == ref64.shape else float("nan")
    return bool(e <= b), e, e_f32, b


# ---- mutants of the float32 oracle: what the comparison must be able to reject ----------------------------------------

def _offsets(c, jtr, trans):
    """The per-frame offset smpl_layer.py:147-155 adds to vertices and joints, from uncentred joints -> f32[B,1,3] | None."""
    if trans is not None and not smpl_ref64.all_zero_f32(trans):
        return np.asarray(trans, F32)[:, None]
    if c.center_idx is not None:
        return -jtr[:, c.center_idx][:, None]
    return None


def _deepest_leaf(parents):
    depth = [0] * J
    for i in range(1, J):
        depth[i] = depth[parents[i]] + 1
    i = max(range(J), key=lambda k: (depth[k], k))
    p = int(parents[i])
    wrong = int(parents[p]) if p > 0 else (1 if i != 1 else 2)     # the grandparent; in a star, a sibling
    return i, p, wrong


MUTANTS = ("drop_last_pose_coefficient", "swap_first_two_weights", "stale_offset", "wrong_parent_at_deepest_level",
           "centre_added", "ignore_a_beta_past_the_10th")


def mutant(name, kind):
    """-> {"verts", "joints"} of oracle.smpl_ref with the defect `kind`, or None where the defect cannot show on the case.
    kind None: the same route with no defect (it must reproduce the oracle bit for bit)."""
    c = BY_NAME[name]
    m, (pose, betas, trans), _, _ = references(name)
    m = dict(m)
    B = c.B
    R = smpl_ref64.batch_rodrigues(np.asarray(pose, np.float64).reshape(B * J, 3)).reshape(B, J, 3, 3)
    if kind == "drop_last_pose_coefficient":
        if np.abs(R[:, J - 1, 2, 2] - 1).max() < 1e-2:
            return None
        m["posedirs"] = m["posedirs"].copy()
        m["posedirs"][:, :, -1] = 0
    if kind == "swap_first_two_weights":
        if c.nnz_max < 2:
            return None
        w = m["weights"].copy()
        for v in range(c.V):
            nz = np.flatnonzero(w[v])
            if len(nz) >= 2:
                w[v, nz[0]], w[v, nz[1]] = w[v, nz[1]], w[v, nz[0]]
        m["weights"] = w
    if kind == "ignore_a_beta_past_the_10th":
        if c.NB <= 10:
            return None
        betas = betas.copy()
        betas[:, 10] = 0
    verts, jtr = smpl_ref.smpl_forward(oracle_model(m), pose, betas, None, None)      # no offset yet
    if kind == "wrong_parent_at_deepest_level":
        i, p, wrong = _deepest_leaf(m["parents"])
        _, j0, _ = smpl_ref64.rest_joints(m, betas, B)
        G = smpl_ref64.chain(m["parents"], R, j0)
        if np.abs(j0[:, p] - j0[:, wrong]).max() < 1e-3:      # one vertex: every rest joint is that vertex
            return None
        delta = np.einsum("brc,bc->br", G[:, p, :3, :3], j0[:, p] - j0[:, wrong]).astype(F32)     # joint i is a leaf
        jtr = jtr.copy()
        jtr[:, i] += delta
        verts = verts + m["weights"][None, :, i, None] * delta[:, None, :]
    off = _offsets(c, jtr, trans)
    if kind == "stale_offset":
        if off is None or B < 2 or np.abs(off - np.roll(off, 1, axis=0)).max() < 1e-3:    # (the root's rest position without betas)
            return None
        off = np.roll(off, 1, axis=0)
    if kind == "centre_added":
        if off is None or (trans is not None and not smpl_ref64.all_zero_f32(trans)):
            return None
        off = -off
    if off is not None:
        verts, jtr = verts + off, jtr + off
    return {"verts": verts.astype(F32), "joints": jtr.astype(F32)}
