"""Generate the golden fixtures under tests/golden/ by running the REFERENCE's own Python.

Run in the build container only (needs /root/reference, which never travels):

    python tests/golden/make_golden.py

What is imported from the reference, unmodified (sys.path ordered as main/__init_path.py:16-32):
  * smplpytorch.pytorch.{smpl_layer,rodrigues_layer,tensutils}  -> SMPL_Layer.forward, batch_rodrigues
    (SMPL_Layer.__init__ needs chumpy + the licensed .pkl, so the instance is made with __new__ and
    the seven buffers are registered from a seeded synthetic model of the same layout)
  * coord_utils  -> get_joint_cam, axis_angle_to_euler_angle, rotationMatrixToEulerAngles
    (it does `import cv2`; OpenCV is absent here, so oracle.rodrigues_cv.Rodrigues is installed as
    the `cv2` module: the Euler arithmetic is the reference's, the Rodrigues part is ours)
  * reba.REBA, rula.RULA  -> scores and log_score (scores.npz; score_probes.npz over the probe set of tests/score_cases.py)
  * core.base  -> Predictor.get_pose_estimation_results (base.py:211-240) and Predictor.post_processing
    (base.py:242-271), called UNBOUND on a plain namespace holding oracle.hmr_ref as `spin_model` (SPIN's source is not in
    the tree) and the synthetic SMPL holder.  `import core.base` needs modules the container lacks -- easydict,
    multi_person_tracker(.data), SPIN's `models`, torchvision(.transforms(.functional)) -- so EMPTY module objects of those
    names are put in sys.modules first (easydict gets the attribute-dict its name stands for, nothing else has a body);
    neither function touches one of them except cv2.Rodrigues, which is the oracle's as above.  driver_loop.npz therefore
    pins the reference's LOOP (batches of 8, betas / camera dropped (Q3), the in-place root overwrite (Q5), dtypes, the
    order of frames) and its aggregation (sort, NaN top-10 % below ten frames (Q20), scipy's mode), not the encoder.

Inputs come from poserisk_release_amd.synth (NumPy PCG64, fixed seeds) and are stored next to the
expected outputs, so the fixtures are self-contained data.
"""
import json
import os
import sys
import types

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.abspath(os.path.join(HERE, "..", ".."))
REF = os.environ.get("POSERISK_REFERENCE", "/root/reference")
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from oracle import rodrigues_cv  # noqa: E402
from poserisk_release_amd import synth  # noqa: E402


def _reference_paths():
    for sub in ("lib", "data", os.path.join("lib", "utils"), os.path.join("lib", "smplpytorch")):
        p = os.path.join(REF, sub)
        if p not in sys.path:
            sys.path.insert(0, p)
    cv2 = types.ModuleType("cv2")
    cv2.Rodrigues = rodrigues_cv.Rodrigues
    sys.modules["cv2"] = cv2


def _ref_smpl_layer(model):
    from smplpytorch.pytorch.smpl_layer import SMPL_Layer
    layer = SMPL_Layer.__new__(SMPL_Layer)
    torch.nn.Module.__init__(layer)
    layer.center_idx = None
    layer.gender = "neutral"
    layer.register_buffer("th_betas", torch.tensor(model["model_betas"]).unsqueeze(0))
    layer.register_buffer("th_shapedirs", torch.tensor(model["shapedirs"]))
    layer.register_buffer("th_posedirs", torch.tensor(model["posedirs"]))
    layer.register_buffer("th_v_template", torch.tensor(model["v_template"]).unsqueeze(0))
    layer.register_buffer("th_J_regressor", torch.tensor(model["J_regressor"]))
    layer.register_buffer("th_weights", torch.tensor(model["weights"]))
    layer.kintree_parents = [int(p) for p in model["parents"]]
    layer.kintree_parents[0] = -1
    layer.num_joints = 24
    return layer


def gen_smpl():
    out = {}
    small = synth.smpl_model(V=97, seed=2)
    dense = synth.smpl_model(V=64, seed=7, dense_weights=True, model_betas=np.linspace(-0.5, 0.5, 10))
    layers = {"small": (small, _ref_smpl_layer(small)), "dense": (dense, _ref_smpl_layer(dense))}
    for tag, (model, layer) in layers.items():
        for B in (1, 4):
            pose = synth.poses(B, seed=10 + B)
            for bt, betas in (("zero", np.zeros((B, 10), np.float32)), ("rand", synth.betas(B, seed=20 + B))):
                with torch.no_grad():
                    v, j = layer(torch.tensor(pose), torch.tensor(betas))
                out[f"{tag}_B{B}_{bt}_pose"] = pose
                out[f"{tag}_B{B}_{bt}_betas"] = betas
                out[f"{tag}_B{B}_{bt}_verts"] = v.numpy()
                out[f"{tag}_B{B}_{bt}_joints"] = j.numpy()
    # translation branch (smpl_layer.py:153-155)
    pose = synth.poses(2, seed=31)
    trans = np.array([[0.1, -0.2, 0.3], [1.0, 2.0, -3.0]], np.float32)
    with torch.no_grad():
        v, j = layers["small"][1](torch.tensor(pose), torch.tensor(synth.betas(2, seed=32)), torch.tensor(trans))
    out.update(trans_pose=pose, trans_betas=synth.betas(2, seed=32), trans_trans=trans, trans_verts=v.numpy(),
               trans_joints=j.numpy())
    # full-size model: strided vertex sample + all joints (keeps the fixture small)
    full = synth.smpl_model(V=6890, seed=2)
    lf = _ref_smpl_layer(full)
    pose = synth.poses(3, seed=41)
    betas = synth.betas(3, seed=42)
    with torch.no_grad():
        v, j = lf(torch.tensor(pose), torch.tensor(betas))
    out.update(full_pose=pose, full_betas=betas, full_verts_stride53=v.numpy()[:, ::53], full_joints=j.numpy())
    np.savez_compressed(os.path.join(HERE, "smpl.npz"), **out)

    # G2: get_joint_cam on the small and full models (captures Q4/Q5: root overwrite, in-place mutation)
    import coord_utils
    g2 = {}
    for tag, layer in (("small", layers["small"][1]), ("full", lf)):
        holder = types.SimpleNamespace(layer={"neutral": layer})
        aa = synth.poses(5, seed=51).reshape(5, 24, 3)
        aa_in = aa.copy()
        with torch.no_grad():
            jc = coord_utils.get_joint_cam(aa, holder)
        g2[f"{tag}_axis_angle_in"] = aa_in
        g2[f"{tag}_axis_angle_after"] = aa
        g2[f"{tag}_joint_cam"] = jc.astype(np.float32)
    np.savez_compressed(os.path.join(HERE, "joint_cam.npz"), **g2)

    # G3: batch_rodrigues incl. zero / tiny vectors (Q8)
    from smplpytorch.pytorch.rodrigues_layer import batch_rodrigues
    v = np.concatenate([synth.poses(8, seed=61).reshape(-1, 3)[:40],
                        np.zeros((1, 3), np.float32), np.full((1, 3), 1e-9, np.float32),
                        np.array([[1e-6, 0, 0], [0, -1e-7, 2e-7], [3.14, 0, 0], [0, 3.1415927, 0]], np.float32)])
    with torch.no_grad():
        r = batch_rodrigues(torch.tensor(v)).numpy()
    np.savez_compressed(os.path.join(HERE, "rodrigues.npz"), axisang=v, rotmat=r)


def gen_smpl_sweep():
    """smpl_sweep.npz: the reference's SMPL_Layer on the small models of tests/smpl_cases.py -- the centring branch, a
    translation given / zero / absent, large and exactly periodic angles, betas and trans whose squares underflow, other
    kinematic trees and weight counts.  Inputs and outputs are stored; the models come from their seeds."""
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import smpl_cases
    out = {}
    for name, spec in smpl_cases.FIXTURES.items():
        layer = _ref_smpl_layer(smpl_cases.fixture_model(name))
        layer.center_idx = spec["center_idx"]
        pose, betas, trans = smpl_cases.fixture_inputs(name)
        args = [torch.tensor(pose), torch.tensor(betas)] + ([torch.tensor(trans)] if trans is not None else [])
        with torch.no_grad():
            v, j = layer(*args)
        out[f"{name}_pose"], out[f"{name}_betas"] = pose, betas
        if trans is not None:
            out[f"{name}_trans"] = trans
        out[f"{name}_verts"], out[f"{name}_joints"] = v.numpy(), j.numpy()
    np.savez_compressed(os.path.join(HERE, "smpl_sweep.npz"), **out)


def gen_euler():
    import coord_utils
    rot = synth.rotmats(40, seed=5)
    # near-gimbal and special rotations appended to frame 0
    def rz(a): return np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
    def ry(a): return np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    def rx(a): return np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])
    specials = [np.eye(3), ry(np.pi / 2 - 1e-4), ry(-np.pi / 2 + 1e-4), rx(np.pi - 1e-7), rz(np.pi - 1e-3),
                rx(1e-7), rz(0.3) @ ry(1.5) @ rx(-2.0), rx(3.14), ry(np.pi / 2), rz(np.pi), rx(np.pi) @ rz(0.5),
                ry(np.pi - 1e-6)]
    for i, m in enumerate(specials):
        rot[0, i] = m.astype(np.float32)
    aa, eul = [], []
    for fr in rot:
        p = coord_utils.rot_to_angle(fr)
        aa.append(p)
        eul.append(coord_utils.axis_angle_to_euler_angle(p))
    R = np.stack([rodrigues_cv.rotvec_to_rotmat(v) for v in np.stack(aa).reshape(-1, 3)])
    e_direct = np.stack([coord_utils.rotationMatrixToEulerAngles(m) for m in R])
    np.savez_compressed(os.path.join(HERE, "euler.npz"), rotmat=rot, axis_angle=np.stack(aa).astype(np.float32),
                        euler_deg=np.stack(eul), rotmat_from_aa=R, euler_rad_direct=e_direct)


def threshold_grid(rng):
    """Angles straddling every constant the rules compare against (+-eps and exact)."""
    consts = [0, 1, 5, 10, 15, 20, 30, 45, 60, 70, 90, 100, 110]
    vals = []
    for c in consts:
        for s in (1, -1):
            for d in (-0.5, -1e-9, 0.0, 1e-9, 0.5):
                vals.append(s * c + d)
    vals = np.array(sorted(set(vals)))
    n = 3000
    pose = rng.choice(vals, size=(n, 24, 3))
    return pose.astype(np.float64)


def gen_scores():
    from reba import REBA
    from rula import RULA
    rng = np.random.Generator(np.random.PCG64(77))
    pose = np.concatenate([rng.uniform(-180, 180, (1500, 24, 3)), rng.normal(0, 40, (1500, 24, 3)),
                           threshold_grid(rng)])
    pose[0] = np.nan  # comparisons with NaN all fail -> trailing else everywhere
    infos = {
        "example": json.load(open(os.path.join(REF, "example", "additional_information.json"))),
        "default": json.load(open(os.path.join(REF, "main", "default_information.json"))),
    }
    infos["loaded"] = {"REBA": {"Legs_bilateral_weight_bearing/walking": 2, "Sitting": 1, "Load/Force Score": 2,
                                "Arm_supported_leaning_L": 1, "Arm_supported_leaning_R": 0, "Coupling": 2,
                                "Activity_Score": 1},
                       "RULA": {"Arm_supported_leaning_L": 1, "Arm_supported_leaning_R": 1, "A_Muscle_use_L": 1,
                                "A_Muscle_use_R": 0, "A_Load/Force_L": 2, "A_Load/Force_R": 3,
                                "Legs_bilateral_weight_bearing": 2, "B_Muscle_use": 1, "B_Load/Force": 2}}
    out = {"pose": pose, "infos_json": np.array(json.dumps(infos))}
    jc = np.zeros((pose.shape[0], 24, 3), np.float32)

    def pairs(s):
        return [int(x) for x in s.split(",")]

    for name, info in infos.items():
        r = REBA(False)(pose, jc, info)
        out[f"reba_{name}"] = np.array([[d["score"], *d["log_score"][:3], *pairs(d["log_score"][3]),
                                         *pairs(d["log_score"][4]), *pairs(d["log_score"][5])] for d in r], np.int32)
        u = RULA(False)(pose, jc, info)
        out[f"rula_{name}"] = np.array([[d["score"], *pairs(d["log_score"][0]), *pairs(d["log_score"][1]),
                                         *pairs(d["log_score"][2]), *pairs(d["log_score"][3]),
                                         *d["log_score"][4:]] for d in u], np.int32)
    # debug angle logs (reba.py:48,77-79 / rula.py:64,94-96) for the first frames after the NaN one
    rd, ud = REBA(True), RULA(True)
    rd(pose[1:9], jc[1:9], infos["example"]); ud(pose[1:9], jc[1:9], infos["example"])
    out["reba_debug_log_json"] = np.array(json.dumps(rd.log))
    out["rula_debug_log_json"] = np.array(json.dumps(ud.log))
    # action levels (reba.py:83-104, rula.py:100-118)
    out["reba_action"] = np.array([REBA().action_level(s)[0] or 0 for s in range(1, 16)], np.int32)
    out["rula_action"] = np.array([RULA().action_level(s)[0] or 0 for s in range(1, 10)], np.int32)
    # every committed file stays under 1 MiB: the poses (3.5 MB of float64) go in row chunks beside scores.npz, which
    # tests/conftest.py's golden() joins again
    pose = out.pop("pose")
    np.savez_compressed(os.path.join(HERE, "scores.npz"), **out)
    for i, s in enumerate(range(0, len(pose), 1500)):
        np.savez_compressed(os.path.join(HERE, f"scores.pose.{i}.npz"), pose=pose[s:s + 1500])


def gen_score_probes(out_dir=HERE):
    """score_probes.npz: the reference's REBA(False) / RULA(False) over every (pose block, info) pair of tests/score_cases.py
    -- every rule-class product, every special value, every table cell under shifts that cross table C.  Poses, infos and
    pairs are stored beside the results, so the fixture is self-contained data; results are int8 in the kernels' column
    order, one row per (pair, pose), pairs in order."""
    from reba import REBA
    from rula import RULA
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import score_cases
    pose, blocks, infos, pairs = score_cases.build()
    jc = np.zeros((len(pose), 24, 3), np.float32)

    def ints(s):
        return [int(x) for x in s.split(",")]

    reba, rula = [], []
    for block, i in pairs:
        a, b = blocks[block]
        for d in REBA(False)(pose[a:b], jc[a:b], infos[i]):
            reba.append([d["score"], *d["log_score"][:3], *ints(d["log_score"][3]), *ints(d["log_score"][4]),
                         *ints(d["log_score"][5])])
        for d in RULA(False)(pose[a:b], jc[a:b], infos[i]):
            rula.append([d["score"], *ints(d["log_score"][0]), *ints(d["log_score"][1]), *ints(d["log_score"][2]),
                         *ints(d["log_score"][3]), *d["log_score"][4:]])
    reba, rula = np.array(reba, np.int64), np.array(rula, np.int64)
    assert np.abs(reba).max() < 128 and np.abs(rula).max() < 128
    np.savez_compressed(os.path.join(out_dir, "score_probes.npz"), infos_json=np.array(json.dumps(infos)),
                        blocks_json=np.array(json.dumps(blocks)),
                        pairs=np.array([[*blocks[b], i] for b, i in pairs], np.int32),
                        pair_blocks_json=np.array(json.dumps([b for b, _ in pairs])),
                        reba=reba.astype(np.int8), rula=rula.astype(np.int8), pose=pose)
    # few distinct doubles: the poses compress to a tenth, so the one file stays far below 1 MiB and needs no row chunks
    assert os.path.getsize(os.path.join(out_dir, "score_probes.npz")) < 1 << 20


def _import_reference_core_base():
    """`import core.base` as main/run.py:7 reaches it, with empty modules standing where the container lacks a package."""
    os.environ.setdefault("MPLBACKEND", "Agg")

    class EasyDict(dict):                      # what `from easydict import EasyDict as edict` (config.py:5) is used for
        __getattr__ = dict.__getitem__
        __setattr__ = dict.__setitem__

    def empty(name, **attrs):
        if name in sys.modules and name != "cv2":
            return sys.modules[name]
        m = sys.modules.get(name) or types.ModuleType(name)
        for k, v in attrs.items():
            setattr(m, k, v)
        sys.modules[name] = m
        return m

    empty("easydict", EasyDict=EasyDict)
    mpt = empty("multi_person_tracker", MPT=None)
    mpt.data = empty("multi_person_tracker.data", video_to_images=None)
    empty("models", hmr=None)
    tv = empty("torchvision")
    tv.transforms = empty("torchvision.transforms")
    tv.transforms.functional = empty("torchvision.transforms.functional", to_tensor=None)
    import core.base as ref_base
    return ref_base


DRIVER_LOOP_FRAMES = 14        # batches of 8 and 6: the ragged last batch of base.py:218
DRIVER_LOOP_CROP_SEED, DRIVER_LOOP_WEIGHT_SEED, DRIVER_LOOP_SMPL_SEED = 71, 1, 2


def gen_driver_loop():
    """a15 / a14 from the reference's own functions."""
    import tempfile
    from oracle import hmr_ref
    ref_base = _import_reference_core_base()
    from reba import REBA
    from rula import RULA
    sd = synth.hmr_state_dict(seed=DRIVER_LOOP_WEIGHT_SEED)
    crops = synth.crops(DRIVER_LOOP_FRAMES, seed=DRIVER_LOOP_CROP_SEED)
    model = synth.smpl_model(V=6890, seed=DRIVER_LOOP_SMPL_SEED)
    me = types.SimpleNamespace(spin_model=hmr_ref.build(sd), device=torch.device("cpu"),
                               smpl_model=types.SimpleNamespace(layer={"neutral": _ref_smpl_layer(model)}))
    bs = 8                                                   # lib/core/config.py:32
    loader = [torch.tensor(crops[i:i + bs]) for i in range(0, len(crops), bs)]
    result, joint_cam, images, debug_result = ref_base.Predictor.get_pose_estimation_results(me, loader)
    out = dict(n_frames=np.int32(DRIVER_LOOP_FRAMES), batch_size=np.int32(bs),
               seeds=np.array([DRIVER_LOOP_CROP_SEED, DRIVER_LOOP_WEIGHT_SEED, DRIVER_LOOP_SMPL_SEED], np.int32),
               result=result, joint_cam=joint_cam, debug_result=debug_result,
               dtypes_json=np.array(json.dumps(dict(result=str(result.dtype), joint_cam=str(joint_cam.dtype),
                                                    images=str(images.dtype), debug_result=str(debug_result.dtype)))),
               images_shape=np.array(images.shape, np.int32), images_equal_crops=np.bool_(np.array_equal(images, crops)))
    # the scorers on the loop's output, as base.py:151,168 call them, then post_processing
    info = json.load(open(os.path.join(REF, "example", "additional_information.json")))
    with tempfile.TemporaryDirectory() as tmp:
        for title, cls in (("REBA", REBA), ("RULA", RULA)):
            scorer = cls(False)
            res = scorer(result, joint_cam, info)
            final, scores_log, logs = ref_base.Predictor.post_processing(
                me, res, scorer.eval_items, (0, np.arange(len(res)), len(res)), tmp, title=title)
            out[f"{title.lower()}_scores"] = np.asarray(scores_log)
            out[f"{title.lower()}_final"] = np.array(final, np.float64)
            out[f"{title.lower()}_logs_json"] = np.array(json.dumps(np.asarray(logs).tolist()))
            assert os.path.isfile(os.path.join(tmp, title + "_score.png"))
        # aggregation alone on score vectors of 5, 10 and 101 frames (Q20: the top-10 % mean of fewer than ten is NaN)
        rng = np.random.Generator(np.random.PCG64(88))
        for n in (5, 10, 101):
            sc = rng.integers(1, 13, n)
            res = [dict(score=np.int64(v), log_score=[int(v), 0, 0, "0,0", "0,0", "0,0"]) for v in sc]
            final, scores_log, logs = ref_base.Predictor.post_processing(
                me, res, None, (0, np.arange(n), n), tmp, title=f"N{n}")
            assert np.array_equal(scores_log, sc)
            out[f"agg{n}_scores"] = sc.astype(np.int64)
            out[f"agg{n}_final"] = np.array(final, np.float64)
            out[f"agg{n}_final_types_json"] = np.array(json.dumps([type(v).__name__ for v in final]))
    np.savez_compressed(os.path.join(HERE, "driver_loop.npz"), **out)


if __name__ == "__main__":
    _reference_paths()
    gen_smpl()
    gen_smpl_sweep()
    gen_euler()
    gen_scores()
    gen_score_probes()
    gen_driver_loop()
    for f in sorted(os.listdir(HERE)):
        if f.endswith(".npz"):
            print(f, os.path.getsize(os.path.join(HERE, f)))
