"""GPU: pr_smooth_tracks (csrc/smooth.hip) over every case of tests/smooth_cases.py against the float64 restatement of its
contract (tests/smooth_ref.py), every tensor between guard bands; what smoothing does to a planted one-frame outlier's REBA
score; and the Predictor's two knobs end to end, on one rank and on two."""
import ctypes as C
import json
import os
import pickle
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

import guard_band as gb
import smooth_cases as sc
from conftest import REPO, measured
from poserisk_release_amd import _lib, ops, smooth, synth

pytestmark = pytest.mark.gpu


def _call(c, i, o):
    lib = _lib.load()
    N = len(c["frame_no"])
    ts = c["track_start"]
    ptr = lambda d, k: d[k].data_ptr() if k in d else None
    _lib.check(lib.pr_smooth_tracks(C.byref(_lib.SmoothParams(c["m"], 0, c["sigma"])),
                                    C.byref(_lib.SmoothInputs(ptr(i, "rotmat"), ptr(i, "betas"), ptr(i, "cam"))), i["frame_no"].data_ptr(),
                                    (C.c_int * len(ts))(*ts.tolist()), len(ts) - 1, N,
                                    C.byref(_lib.SmoothOutputs(ptr(o, "rotmat"), ptr(o, "betas"), ptr(o, "cam"), ptr(o, "replaced"))),
                                    ptr(o, "status"), ptr(o, "workspace"), torch.cuda.current_stream().cuda_stream), "pr_smooth_tracks")


# ---- the contract, through the C ABI, between guard bands -------------------------------------------------------------------
def _run_guarded(gpu_device, name):
    """One case or sweep problem through the C entry between guard bands, checked against its reference -> the worst
    rotation error."""
    lib = _lib.load()
    assert lib.pr_smooth_tile_rows() == sc.TILE
    c = sc.case(name)
    N = len(c["frame_no"])
    ins = {k: torch.from_numpy(c[k]).to(gpu_device) for k in ("rotmat", "betas", "cam", "frame_no") if c[k] is not None}
    outs = {"rotmat": ((N, 24, 3, 3), torch.float32), "status": ((N,), torch.int32), "replaced": ((N,), torch.int32)}
    if c["betas"] is not None:
        outs["betas"] = ((N, 10), torch.float32)
    if c["cam"] is not None:
        outs["cam"] = ((N, 3), torch.float32)
    if c["m"] > 0 and c["sigma"] > 0:
        outs["workspace"] = ((lib.pr_smooth_workspace_bytes(N, c["betas"] is not None, c["cam"] is not None) // 4,), torch.float32)
    # the workspace's size is rounded up to 256 bytes: its tail is never written
    # a case that plants NaNs says where its reference holds one (stage 1's output for the workspace); nowhere else may one be
    nans = None
    if not c["rotations"]:
        ref = sc.reference(name)
        nans = {k: np.isnan(np.asarray(ref[k])) for k in ("rotmat", "betas", "cam")}
        if "workspace" in outs:
            ws = np.concatenate([np.isnan(ref["stage1"][k]).reshape(-1) for k in ("rotmat", "cam", "betas")])
            nans["workspace"] = np.concatenate([ws, np.zeros(outs["workspace"][0][0] - ws.size, bool)])
    got = gb.run_guarded(lambda i, o: _call(c, i, o), ins, outs, may_hold_canary=("workspace",), nan_expected=nans)
    host = {k: (got[k].cpu().numpy() if k in got else None) for k in ("rotmat", "betas", "cam", "status", "replaced")}
    worst = sc.check(name, host)
    # orthonormal enough for the next stage: pose_to_euler's isRotationMatrix and round-trip checks pass on every row -- of
    # every case that holds rotations throughout (all but those that plant NaNs and infinities)
    if c["rotations"]:
        _, _, st = ops.pose_to_euler(got["rotmat"])
        assert not st.cpu().numpy().any()
    else:
        assert name.startswith("nonfinite_")
    return worst


@pytest.mark.parametrize("name", sc.NAMES)
def test_every_case_matches_the_reference_inside_its_guard_bands(gpu_device, name):
    """Inputs between NaN / 0x7fffffff guards, outputs, status, replaced and the workspace between canary guards
    (tests/guard_band.py): a window that left its track's rows at a tile's or a tensor's edge would read a guard (a NaN
    reaches the output, a frame number of 0x7fffffff is no member), a store outside a tensor lands in one."""
    measured(f"smooth_rot_err[{name}]", _run_guarded(gpu_device, name), sc.ROT_TOL)


SWEEP_BLOCK = 10


@pytest.mark.parametrize("block", range(0, sc.SWEEP, SWEEP_BLOCK))
def test_the_seeded_sweep_matches_the_reference_inside_its_guard_bands(gpu_device, block):
    """Ten problems of smooth_cases.sweep_problem a test id, each as the cases above."""
    worst = max(_run_guarded(gpu_device, sc.sweep_name(q)) for q in range(block, min(block + SWEEP_BLOCK, sc.SWEEP)))
    measured(f"smooth_rot_err[sweep_{block}]", worst, sc.ROT_TOL)


def test_smooth_tracks_is_capturable(gpu_device):
    """Both stages with the workspace, captured once on a side stream (one stream, no branches) and replayed twice with every
    input overwritten in place in between: each replay gives the eager call's bits for the inputs it found."""
    c = sc.case("mixed_m2_s1.5")
    N = len(c["frame_no"])
    lib = _lib.load()
    second = {k: np.roll(c[k], 7, axis=0) for k in ("rotmat", "betas", "cam")}
    second["frame_no"] = c["frame_no"].copy()
    second["frame_no"][50:90] += 2                                        # (rows 50 .. 89 of the first track: a new gap)
    sets = [{k: torch.from_numpy(np.ascontiguousarray(src[k])).to(gpu_device) for k in ("rotmat", "betas", "cam", "frame_no")} for src in (c, second)]
    ins = {k: torch.empty_like(v) for k, v in sets[0].items()}
    new = lambda: {"rotmat": torch.zeros((N, 24, 3, 3), device=gpu_device), "betas": torch.zeros((N, 10), device=gpu_device),
                   "cam": torch.zeros((N, 3), device=gpu_device), "status": torch.full((N,), -1, dtype=torch.int32, device=gpu_device),
                   "replaced": torch.full((N,), -1, dtype=torch.int32, device=gpu_device),
                   "workspace": torch.zeros((lib.pr_smooth_workspace_bytes(N, 1, 1) // 4,), device=gpu_device)}
    eager = []
    for given in sets:
        for k in ins:
            ins[k].copy_(given[k])
        outs = new()
        _call(c, ins, outs)
        eager.append({k: outs[k].clone() for k in ("rotmat", "betas", "cam", "status", "replaced")})
    assert not torch.equal(eager[0]["rotmat"], eager[1]["rotmat"]) and not torch.equal(eager[0]["replaced"], eager[1]["replaced"])
    outs = new()
    for k in ins:
        ins[k].copy_(sets[0][k])
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        _call(c, ins, outs)
    for given, want in zip(sets, eager):
        for k in ins:
            ins[k].copy_(given[k])
        for k in want:
            outs[k].fill_(-1)
        g.replay()
        torch.cuda.synchronize()
        for k in want:
            assert torch.equal(outs[k].view(torch.int32), want[k].view(torch.int32)), k


def test_a_track_smoothed_alone_and_among_others_gives_the_same_bits(gpu_device):
    c = sc.case("mixed_m2_s1.5")
    dev = lambda a: torch.from_numpy(a).to(gpu_device)
    whole = smooth.smooth_tracks(dev(c["rotmat"]), c["frame_no"], c["track_start"], 2, 1.5, betas=dev(c["betas"]), cam=dev(c["cam"]))
    for a, b in zip(c["track_start"][:-1], c["track_start"][1:]):       # alone, every track starts a tile of its own
        one = smooth.smooth_tracks(dev(c["rotmat"][a:b]), torch.from_numpy(c["frame_no"][a:b]).to(gpu_device), [0, b - a], 2, 1.5,
                                   betas=dev(c["betas"][a:b]), cam=dev(c["cam"][a:b]))
        for k in ("rotmat", "betas", "cam", "status", "replaced"):
            assert torch.equal(one[k].view(torch.int32), whole[k][a:b].view(torch.int32)), (k, a, b)
    # and more tracks than one launch carries: 300 tracks of one row each come back unchanged, with both stages
    n = _lib.load().pr_smooth_tile_rows() * 9 + 12
    rot = dev(np.tile(c["rotmat"], (3, 1, 1, 1))[:n])
    many = smooth.smooth_tracks(rot, np.zeros(n, np.int64), np.arange(n + 1), 2, 1.5)
    assert n > 256 and torch.equal(many["rotmat"].view(torch.int32), rot.view(torch.int32)) and not many["status"].any()
    assert many["betas"] is None and many["cam"] is None and not many["replaced"].any()
    empty = smooth.smooth_tracks(rot[:0], np.zeros(0, np.int64), [0], 2, 1.5)
    assert empty["rotmat"].shape == (0, 24, 3, 3) and empty["status"].shape == (0,)


# ---- what it is for: a one-frame outlier no longer sets the score ----------------------------------------------------------------
def test_a_one_frame_trunk_flexion_no_longer_sets_the_maximum(gpu_device):
    from oracle.risk_tables import J
    rng = np.random.default_rng(12)     # a base pose none of whose angles lies within the jitter of a rule's threshold
    n, planted = 21, 9
    aa = rng.uniform(-0.3, 0.3, (1, 24, 3)) + rng.normal(0, 0.002, (n, 24, 3))      # near-static: 0.1 degree of jitter
    aa[:, J["Torso"]] = rng.normal(0, 0.002, (n, 3))                                   # an upright trunk ...
    aa[planted, J["Torso"]] = [np.deg2rad(70.0), 0.0, 0.0]                             # ... bent forward by 70 degrees for one frame
    rot = torch.from_numpy(sc.rodrigues(aa).astype(np.float32)).to(gpu_device)

    def reba(r):
        _, eul, st = ops.pose_to_euler(r)
        assert not st.any()
        return ops.reba(eul, synth.EXAMPLE_INFO["REBA"]).cpu().numpy()
    raw = reba(rot)
    others = np.delete(np.arange(n), planted)
    assert (raw[others] == raw[others[0]]).all()                                       # the neighbours agree: the pose is static
    assert raw[planted, 1] > raw[planted - 1, 1] and raw[planted, 1] > raw[planted + 1, 1]          # the trunk sub-score
    assert raw[:, 0].max() == raw[planted, 0] > raw[others, 0].max()                   # ... sets MAX Score on its own
    sm = smooth.smooth_tracks(rot, np.arange(n), [0, n], 1, 0.0)
    out = reba(sm["rotmat"])
    assert (out[planted] == out[planted - 1]).all() and (out[planted] == out[planted + 1]).all()
    assert out[:, 0].max() == raw[others, 0].max() and out[planted, 1] == raw[planted - 1, 1]
    assert int(sm["replaced"][planted]) >> J["Torso"] & 1 and not sm["status"].any()


# ---- the Predictor -----------------------------------------------------------------------------------------------------------------
N_FRAMES = 24
M, SIGMA = 2, 1.5


@pytest.fixture(scope="module")
def clip():
    """24 frames of 160 x 120 and three tracks of 24, 17 (with a gap of 3 frames) and 9 frames, largest box first."""
    rng = np.random.default_rng(9)
    frames = rng.integers(0, 256, (N_FRAMES, 120, 160, 3), dtype=np.uint8)
    tr = {}
    for pid, (fidx, w, h, x) in {5: (np.arange(24), 50, 100, 40), 2: (np.r_[4:12, 15:24], 40, 80, 90), 11: (np.arange(15, 24), 30, 60, 130)}.items():
        tr[pid] = {'bbox': np.stack([np.array([x + i, 60 - i % 3, w, h], np.float32) for i in range(len(fidx))]), 'frames': fidx}
    return frames, tr


def _predictor(gpu_device, score_type="REBA,RULA", **knobs):
    from poserisk_release_amd import dropin
    dropin.install()
    from core import base
    from models import hmr
    from smpl import SMPL
    model = hmr()
    model.load_state_dict(synth.hmr_state_dict(seed=1), strict=False)
    smpl = SMPL(models={"neutral": synth.smpl_model(V=6890, seed=2)}, device=gpu_device)
    args = types.SimpleNamespace(gpu="0", type=score_type, debug=False, debug_joints="", debug_frame=-1, **knobs)
    return base.Predictor(args, spin_model=model, smpl_model=smpl, batch_size=16)


def _same(a, b, what, skip=()):
    assert [k for k in a if k not in skip] == [k for k in b if k not in skip], (what, list(a), list(b))
    for k in a:
        if k in skip:
            continue
        if k in ("reba", "rula"):
            (fa, sa, la, aa), (fb, sb, lb, ab) = a[k], b[k]
            assert np.array_equal(np.array(fa), np.array(fb), equal_nan=True) and np.array_equal(sa, sb) and np.array_equal(la, lb) and aa == ab, (what, k)
        elif k == "add_info":
            assert a[k] == b[k]
        else:
            assert np.asarray(a[k]).dtype == np.asarray(b[k]).dtype and np.array_equal(a[k], b[k]), (what, k)


@pytest.fixture(scope="module")
def unsmoothed(gpu_device, clip):
    frames, tr = clip
    return _predictor(gpu_device).score_people(frames, tr, synth.EXAMPLE_INFO, with_smpl_params=True)


def test_with_both_knobs_at_zero_every_array_is_the_knobs_off_run(gpu_device, clip, unsmoothed):
    frames, tr = clip
    zero = _predictor(gpu_device, smooth_median_radius=0, smooth_sigma=0.0).score_people(frames, tr, synth.EXAMPLE_INFO, with_smpl_params=True)
    assert zero["ids"] == unsmoothed["ids"] == [5, 2, 11]
    for a, b in zip(zero["people"], unsmoothed["people"]):
        _same(a, b, "knobs 0")
        assert "smooth" not in a


def test_the_knobs_smooth_every_person_and_rescore_from_the_smoothed_rotations(gpu_device, clip, unsmoothed, tmp_path, monkeypatch):
    frames, tr = clip
    pred = _predictor(gpu_device, smooth_median_radius=M, smooth_sigma=SIGMA, persons="all")
    people = pred.score_people(frames, tr, synth.EXAMPLE_INFO, with_smpl_params=True)
    assert people["ids"] == [5, 2, 11]
    layer = pred.smpl_model.layer['neutral']
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(gpu_device)
    changed = 0
    for pid, out, raw in zip(people["ids"], people["people"], unsmoothed["people"]):
        n = len(raw["frames"])
        assert np.array_equal(out["frames"], raw["frames"]) and np.array_equal(out["bboxes"], raw["bboxes"])
        # this person's unsmoothed parameters, smoothed alone: the bits the shared call gave
        sm = smooth.smooth_tracks(dev(raw["rotmat"]), raw["frames"], [0, n], M, SIGMA, betas=dev(raw["betas"]), cam=dev(raw["cam"]))
        for k in ("rotmat", "betas", "cam"):
            assert np.array_equal(out[k].view(np.int32), sm[k].cpu().numpy().view(np.int32)), (pid, k)
        assert np.array_equal(out["smooth"]["status"], sm["status"].cpu().numpy()) and np.array_equal(out["smooth"]["replaced"], sm["replaced"].cpu().numpy())
        assert out["smooth"]["median_radius"] == M and out["smooth"]["sigma"] == SIGMA
        changed += int((out["rotmat"] != raw["rotmat"]).any())
        # the back half again from the smoothed rotations: Euler angles, then joint_cam with its root overwrite
        aa, eul, st = ops.pose_to_euler(sm["rotmat"])
        jc = layer.joint_cam(aa)
        assert not st.any() and np.array_equal(out["result"], eul.cpu().numpy()) and np.array_equal(out["joint_cam"], jc.cpu().numpy())
        assert np.array_equal(out["debug_result"], aa.cpu().numpy()) and (out["debug_result"][:, 0] == np.float32([3.14, 0, 0])).all()
        again = dict(result=out["result"], joint_cam=out["joint_cam"])
        pred._run_scorers(again, synth.EXAMPLE_INFO)
        _same({k: out[k] for k in ("reba", "rula")}, {k: again[k] for k in ("reba", "rula")}, f"person {pid}")
    assert changed == 3
    # score_frames takes the same path: the target is element 0
    target = _predictor(gpu_device, smooth_median_radius=M, smooth_sigma=SIGMA).score_frames(frames, tr, synth.EXAMPLE_INFO, with_smpl_params=True)
    _same(target, people["people"][0], "the target", skip=("smooth",))
    assert np.array_equal(target["smooth"]["status"], people["people"][0]["smooth"]["status"])
    # without with_smpl_params the parameters are asked for internally and not returned
    plain = _predictor(gpu_device, "REBA", smooth_median_radius=M, smooth_sigma=SIGMA).score_frames(frames, tr, synth.EXAMPLE_INFO)
    assert "rotmat" not in plain and "smooth" in plain and np.array_equal(plain["result"], target["result"])
    # __call__ writes smooth.json, only with a knob on
    monkeypatch.setitem(sys.modules, "cv2", None)
    src = tmp_path / "clip"
    src.mkdir()
    np.save(src / "frames.npy", frames)
    with open(src / "tracking.pkl", "wb") as f:
        pickle.dump(tr, f)
    pred.visualize = False
    pred(str(src), "", str(tmp_path / "on"))
    doc = json.loads((tmp_path / "on" / "smooth.json").read_text())
    assert (doc["median_radius"], doc["sigma"], doc["unit"], doc["gaussian_radius"]) == (M, SIGMA, "frames", 5)
    want = []
    for pid, out in zip(people["ids"], people["people"]):
        replaced, fallbacks = smooth.counts(out["smooth"]["status"], out["smooth"]["replaced"])
        want.append(dict(id=pid, n_frames=len(out["frames"]), replaced=replaced, fallbacks=fallbacks))
    assert doc["people"] == want and sum(p["replaced"] for p in want) > 0
    off = _predictor(gpu_device, "REBA", persons="all")
    off.visualize = False
    off(str(src), "", str(tmp_path / "off"))
    assert not (tmp_path / "off" / "smooth.json").exists() and (tmp_path / "off" / "people.json").exists()


def test_two_ranks_smooth_the_gathered_rows_alike(gpu_device, tmp_path):
    """Two ranks sharing the GPU each score a shard, gather once and smooth the same gathered rows: every rank ends with the
    single process' smoothed results, bit for bit (tests/smooth_ranks_child.py)."""
    port = str(35500 + os.getpid() % 2000)
    child = os.path.join(REPO, "tests", "smooth_ranks_child.py")
    procs = [subprocess.Popen([sys.executable, child, REPO, port, str(r)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
             for r in range(2)]
    outs = [p.communicate(timeout=600)[0] for p in procs]
    for p, o in zip(procs, outs):
        assert p.returncode == 0 and "ok" in o, o[-3000:]
