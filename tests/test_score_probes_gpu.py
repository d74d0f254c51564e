"""reba_kernel and rula_kernel on the score probe set (tests/score_cases.py): every rule-class product, every special value
and every table cell, bit for bit against what the reference's own classes gave (tests/golden/score_probes.npz); then the
ways a row reaches the kernels -- any batch size, the drop-in classes, the pipeline's info pointers."""
import json

import numpy as np
import pytest
import torch

import score_cases
import score_probe_checks as ck
from conftest import golden
from oracle import reba_ref, rula_ref
from poserisk_release_amd import dropin, ops, synth
from poserisk_release_amd.hmr import HMR
from poserisk_release_amd.pipeline import FramePipeline
from poserisk_release_amd.smpl_layer import SMPLLayer

pytestmark = pytest.mark.gpu

# packed column -> the rule groups whose angles decide it (the right arm's rules also read the left shoulder: Q13)
_ARM = lambda s: [f"{s}_upper_arm", f"{s}_thorax", "cross"]
REBA_GROUPS = {"trunk": ["torso"], "neck": ["neck"], "leg": ["knees"], "upper_arm L": _ARM("l"), "upper_arm R": _ARM("r"),
               "lower_arm L": ["l_elbow"], "lower_arm R": ["r_elbow"], "wrist L": ["l_wrist"], "wrist R": ["r_wrist"]}
RULA_GROUPS = {"upper_arm L": _ARM("l"), "upper_arm R": _ARM("r"), "lower_arm L": ["l_elbow", "l_thorax"],
               "lower_arm R": ["r_elbow", "r_thorax"], "wrist L": ["l_wrist"], "wrist R": ["r_wrist"],
               "wrist_twist L": ["l_wrist"], "wrist_twist R": ["r_wrist"], "neck": ["neck"], "trunk": ["torso"], "leg": []}
ALL_GROUPS = dict(score_cases.GROUPS, cross=score_cases.CROSS)
SENTINEL = -77


@pytest.fixture(scope="module")
def probes(gpu_device):
    g = golden("score_probes.npz")
    pairs = [(int(a), int(b), int(i)) for a, b, i in g["pairs"]]
    starts = np.concatenate([[0], np.cumsum([b - a for a, b, _ in pairs])])
    return dict(pose=g["pose"], dev=torch.from_numpy(g["pose"]).to(gpu_device), infos=json.loads(str(g["infos_json"])),
                pairs=pairs, pair_blocks=json.loads(str(g["pair_blocks_json"])), starts=starts,
                blocks=json.loads(str(g["blocks_json"])), reba=g["reba"].astype(np.int32), rula=g["rula"].astype(np.int32))


def _stored(p, scorer, block, info):
    """The stored rows of the pair (block, info dict)."""
    n = list(zip(p["pair_blocks"], (i for _, _, i in p["pairs"]))).index((block, p["infos"].index(info)))
    return p[scorer][p["starts"][n]:p["starts"][n + 1]]


def _explain(pose_row, col, groups):
    """The classes of the angles behind a differing column (all groups for the final score)."""
    names = groups.get(col) if col in groups else list(ALL_GROUPS)
    return {n: [(j, k, float(pose_row[ck.J[j], k]), int(c)) for (j, k, th), c in
                zip(ALL_GROUPS[n], ck.class_tuples(pose_row[None], ALL_GROUPS[n])[0])] for n in names}


def test_kernels_match_reference_on_every_pair(probes):
    p = probes
    assert max(b - a for a, b, _ in p["pairs"]) < 5000
    for n, (a, b, i) in enumerate(p["pairs"]):
        info = p["infos"][i]
        for name, fn, cols, groups in (("reba", ops.reba, ck.REBA_COLS, REBA_GROUPS), ("rula", ops.rula, ck.RULA_COLS, RULA_GROUPS)):
            got = fn(p["dev"][a:b], info[name.upper()]).cpu().numpy()
            want = p[name][p["starts"][n]:p["starts"][n + 1]]
            d = ck.first_difference(got, want, cols)
            assert d is None, (name, "pair", n, p["pair_blocks"][n], info[name.upper()], "pose row", a + d[0], "column", d[1],
                               "got", got[d[0]].tolist(), "want", want[d[0]].tolist(),
                               _explain(p["pose"][a + d[0]], d[1], groups))


@pytest.mark.parametrize("N", [1, 63, 64, 65, None])
def test_a_rows_bits_do_not_depend_on_its_batch(probes, gpu_device, N):
    """64 frames a block: the same rows alone, one short of a block, a block, one over, and the whole grid (765 rows: eleven
    blocks and a ragged one); the output lies inside a larger tensor whose rows past N keep their sentinel."""
    p = probes
    info = score_cases.make_info({"Sitting": 1})
    a, b = p["blocks"]["grid"]
    N = b - a if N is None else N
    for name, fn, width in (("reba", ops.reba, 10), ("rula", ops.rula, 12)):
        want = _stored(p, name, "grid", info)[:N]
        big = torch.full((N + 70, width), SENTINEL, dtype=torch.int32, device=gpu_device)
        out = fn(p["dev"][a:a + N], info[name.upper()], out=big[:N])
        assert out.data_ptr() == big.data_ptr()
        got = big.cpu().numpy()
        np.testing.assert_array_equal(got[:N], want)
        assert (got[N:] == SENTINEL).all(), (name, N, np.argwhere(got[N:] != SENTINEL)[:4].tolist())
        # the last rows of the whole batch again, as a batch of their own starting elsewhere in the launch grid
        tail = fn(p["dev"][a + N - 1:a + N], info[name.upper()]).cpu().numpy()
        np.testing.assert_array_equal(tail, want[N - 1:N])


def test_dropin_classes_give_the_stored_scores_and_logs(probes):
    dropin.install()
    import reba
    import rula
    p = probes
    for info in (score_cases.arm_infos()[2], score_cases.arm_infos()[5]):
        for block in ("cells_reba_arm", "cells_rula_arm"):
            a, b = p["blocks"][block]
            rows = np.arange(0, b - a, max(1, (b - a) // 100))     # 108 rows: left-arm, right-arm and both-arm cells
            pose, jc = p["pose"][a + rows], np.zeros((len(rows), 24, 3), np.float32)
            w = _stored(p, "reba", block, info)[rows]
            res = reba.REBA()(pose, jc, info)
            assert [int(r["score"]) for r in res] == w[:, 0].tolist() and isinstance(res[0]["score"], np.int64)
            assert [r["log_score"] for r in res] == [[int(r[1]), int(r[2]), int(r[3]), f"{r[4]},{r[5]}", f"{r[6]},{r[7]}",
                                                      f"{r[8]},{r[9]}"] for r in w]
            w = _stored(p, "rula", block, info)[rows]
            res = rula.RULA()(pose, jc, info)
            assert [int(r["score"]) for r in res] == w[:, 0].tolist() and isinstance(res[0]["score"], np.int64)
            assert [r["log_score"] for r in res] == [[f"{r[1]},{r[2]}", f"{r[3]},{r[4]}", f"{r[5]},{r[6]}", f"{r[7]},{r[8]}",
                                                      int(r[9]), int(r[10]), int(r[11])] for r in w]


def test_pipeline_passes_every_info_field_to_the_kernels(gpu_device):
    """pr_frames_forward takes the two info structs by pointer, not through ops.reba / ops.rula: under two infos that differ
    in every field (and give every field of a struct its own value) its scores are what ops computes from the pipeline's
    own Euler angles under the same info, and what the oracle computes from them."""
    first = score_cases.make_info(
        {"Legs_bilateral_weight_bearing/walking": 1, "Sitting": 2, "Load/Force Score": 3, "Arm_supported_leaning_L": -1,
         "Arm_supported_leaning_R": -2, "Coupling": 4, "Activity_Score": 5},
        {"Arm_supported_leaning_L": -1, "Arm_supported_leaning_R": -2, "A_Muscle_use_L": 1, "A_Muscle_use_R": 2,
         "A_Load/Force_L": 3, "A_Load/Force_R": -3, "Legs_bilateral_weight_bearing": 2, "B_Muscle_use": 4, "B_Load/Force": -4})
    second = score_cases.make_info(
        {"Legs_bilateral_weight_bearing/walking": 3, "Sitting": -1, "Load/Force Score": -2, "Arm_supported_leaning_L": 1,
         "Arm_supported_leaning_R": 2, "Coupling": -3, "Activity_Score": -4},
        {"Arm_supported_leaning_L": 2, "Arm_supported_leaning_R": 1, "A_Muscle_use_L": -1, "A_Muscle_use_R": 3,
         "A_Load/Force_L": 4, "A_Load/Force_R": -2, "Legs_bilateral_weight_bearing": 1, "B_Muscle_use": -3, "B_Load/Force": 5})
    for s in ("REBA", "RULA"):
        assert all(first[s][k] != second[s][k] for k in first[s])
    m = HMR(max_batch=8).to(gpu_device)
    m.load_state_dict(synth.hmr_state_dict(seed=1))
    m.eval()
    layer = SMPLLayer(synth.smpl_model(V=6890, seed=2), device=gpu_device)
    x = torch.from_numpy(synth.crops(2, seed=21)).to(gpu_device)
    seen = []
    for info in (first, second):
        got = {k: v.cpu().numpy() for k, v in FramePipeline(m, layer, info)(x).items()}
        e = torch.from_numpy(got["euler"]).to(gpu_device)
        np.testing.assert_array_equal(got["reba"], ops.reba(e, info["REBA"]).cpu().numpy())
        np.testing.assert_array_equal(got["rula"], ops.rula(e, info["RULA"]).cpu().numpy())
        np.testing.assert_array_equal(got["reba"], reba_ref.reba_packed(got["euler"], info["REBA"]))
        np.testing.assert_array_equal(got["rula"], rula_ref.rula_packed(got["euler"], info["RULA"]))
        seen.append(got)
    np.testing.assert_array_equal(seen[0]["euler"], seen[1]["euler"])
    assert not np.array_equal(seen[0]["reba"], seen[1]["reba"]) and not np.array_equal(seen[0]["rula"], seen[1]["rula"])
