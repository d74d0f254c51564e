"""GPU: pr_activity_tracks (csrc/activity.hip) over every case of tests/activity_cases.py, EQUAL to the float64 restatement of
its contract (tests/activity_ref.py), every tensor between guard bands; pr_reba_rows / pr_rula_rows against the oracle with
the constants raised row by row; and the Predictor's knob end to end, on one rank and on two."""
import ctypes as C
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

import activity_cases as ac
import activity_ref
import guard_band as gb
import score_cases
from conftest import REPO
from oracle import reba_ref, rula_ref
from poserisk_release_amd import _lib, activity, ops, synth

pytestmark = pytest.mark.gpu


def _call(c, i, o):
    lib = _lib.load()
    ts = c["track_start"]
    par = _lib.ActivityParams(c["H"], c["R"], c["G"], c["E"], c["dot_static"], c["dot_move"], c["dot_rapid"])
    _lib.check(lib.pr_activity_tracks(C.byref(par), i["rotmat"].data_ptr(), i["frame_no"].data_ptr(), (C.c_int * len(ts))(*ts.tolist()),
                                      len(ts) - 1, len(c["frame_no"]), o["flags"].data_ptr(), o["adds"].data_ptr(), o["workspace"].data_ptr(),
                                      torch.cuda.current_stream().cuda_stream), "pr_activity_tracks")


# ---- the contract, through the C ABI, between guard bands -------------------------------------------------------------------
def _run_guarded(gpu_device, name):
    """One case or sweep problem through the C entry between guard bands, held to its reference."""
    lib = _lib.load()
    assert lib.pr_activity_tile_rows() == ac.TILE and lib.pr_activity_chunk_rows() == ac.CHUNK
    c = ac.case(name)
    N = len(c["frame_no"])
    if N == 0:                      # nothing to put between guards: the entry returns PR_OK without looking at a pointer
        got = activity.activity_tracks(torch.zeros((0, 24, 3, 3), device=gpu_device), c["frame_no"], c["track_start"], 30.0)
        return ac.check(name, {k: got[k].cpu().numpy() for k in ("flags", "adds")})
    ins = {k: torch.from_numpy(np.array(c[k])).to(gpu_device) for k in ("rotmat", "frame_no")}
    outs = {"flags": ((N, 4), torch.int32), "adds": ((N, 4), torch.int32), "workspace": ((lib.pr_activity_workspace_bytes(N) // 4,), torch.int32)}
    # the workspace's size is rounded up to 256 bytes: its tail is never written
    got = gb.run_guarded(lambda i, o: _call(c, i, o), ins, outs, may_hold_canary=("workspace",))
    ac.check(name, {k: got[k].cpu().numpy() for k in ("flags", "adds")})


@pytest.mark.parametrize("name", ac.NAMES)
def test_every_case_equals_the_reference_inside_its_guard_bands(gpu_device, name):
    """Inputs between NaN / 0x7fffffff guards, flags, adds and the workspace between canary guards (tests/guard_band.py): a chunk
    that left its track's rows at a tile's or a tensor's edge would read a guard (a NaN fails every comparison, a frame number
    of 0x7fffffff is no member), a store outside a tensor lands in one."""
    _run_guarded(gpu_device, name)


SWEEP_BLOCK = 10


@pytest.mark.parametrize("block", range(0, ac.SWEEP, SWEEP_BLOCK))
def test_the_seeded_sweep_equals_the_reference_inside_its_guard_bands(gpu_device, block):
    """Ten problems of activity_cases.sweep_problem a test id, each as the cases above."""
    for q in range(block, min(block + SWEEP_BLOCK, ac.SWEEP)):
        _run_guarded(gpu_device, ac.sweep_name(q))


def test_activity_tracks_is_capturable(gpu_device):
    """The three launches captured once on a side stream (one stream, no branches) and replayed twice with both inputs
    overwritten in place in between: each replay gives the eager call's bits for the inputs it found."""
    c = ac.case("edges")
    N = len(c["frame_no"])
    lib = _lib.load()
    second = dict(rotmat=np.roll(c["rotmat"], 11, axis=0), frame_no=np.array(c["frame_no"]))
    second["frame_no"][70:90] += ac.G0 + 1                                 # a hole in the second track
    sets = [{k: torch.from_numpy(np.ascontiguousarray(src[k])).to(gpu_device) for k in ("rotmat", "frame_no")} for src in (c, second)]
    ins = {k: torch.empty_like(v) for k, v in sets[0].items()}
    new = lambda: {"flags": torch.full((N, 4), -1, dtype=torch.int32, device=gpu_device), "adds": torch.full((N, 4), -1, dtype=torch.int32, device=gpu_device),
                   "workspace": torch.zeros((lib.pr_activity_workspace_bytes(N) // 4,), dtype=torch.int32, device=gpu_device)}
    eager = []
    for given in sets:
        for k in ins:
            ins[k].copy_(given[k])
        outs = new()
        _call(c, ins, outs)
        eager.append({k: outs[k].clone() for k in ("flags", "adds")})
    ac.check("edges", {k: eager[0][k].cpu().numpy() for k in ("flags", "adds")})
    assert not torch.equal(eager[0]["flags"], eager[1]["flags"])
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
            assert torch.equal(outs[k], want[k]), k


def test_a_track_alone_and_among_others_gives_the_same_bits(gpu_device):
    c = ac.case("edges")
    par = dict(hold_seconds=ac.H0, rapid_seconds=ac.R0, gap_seconds=ac.G0, rep_events=ac.E0)       # at 1 fps a second is a frame
    dev = lambda a: torch.from_numpy(np.array(a)).to(gpu_device)
    whole = activity.activity_tracks(dev(c["rotmat"]), c["frame_no"], c["track_start"], 1.0, **par)
    assert (whole["parameters"]["hold_frames"], whole["parameters"]["dot_static"]) == (c["H"], c["dot_static"])
    ac.check("edges", {k: whole[k].cpu().numpy() for k in ("flags", "adds")})
    for a, b in zip(c["track_start"][:-1], c["track_start"][1:]):       # alone, every track starts a tile of its own
        one = activity.activity_tracks(dev(c["rotmat"][a:b]), dev(c["frame_no"][a:b]), [0, b - a], 1.0, **par)
        for k in ("flags", "adds"):
            assert torch.equal(one[k], whole[k][a:b]), (k, a, b)


# ---- the scorers with per-row addends -----------------------------------------------------------------------------------------
def test_the_row_scorers_equal_the_plain_ones_without_rows_and_the_oracle_with(gpu_device):
    """With NULL: pr_reba / pr_rula's bits on every probe pose.  With rows: the oracle called with the constants raised by each
    row's addends -- once per distinct addend over the rows that carry it, which for a scorer that reads one row at a time is
    the row-by-row call."""
    lib = _lib.load()
    pose, _, _, _ = score_cases.build()
    N = len(pose)
    eul = torch.from_numpy(pose).to(gpu_device)
    rng = np.random.default_rng(5)
    act = rng.integers(0, 4, N).astype(np.int32)
    mus = rng.integers(0, 2, (N, 3)).astype(np.int32)
    stream = torch.cuda.current_stream().cuda_stream
    for info in (score_cases.make_info(), score_cases.one_hot_infos()[2], score_cases.one_hot_infos()[0], score_cases.arm_infos()[2],
                 score_cases.ab_infos()[9], synth.EXAMPLE_INFO):
        plain_reba, plain_rula = ops.reba(eul, info["REBA"]).cpu().numpy(), ops.rula(eul, info["RULA"]).cpu().numpy()
        out = torch.full((N, 10), -77, dtype=torch.int32, device=gpu_device)
        _lib.check(lib.pr_reba_rows(eul.data_ptr(), N, _lib.reba_info_struct(info["REBA"]), None, out.data_ptr(), stream), "pr_reba_rows")
        assert np.array_equal(out.cpu().numpy(), plain_reba)
        out = torch.full((N, 12), -77, dtype=torch.int32, device=gpu_device)
        _lib.check(lib.pr_rula_rows(eul.data_ptr(), N, _lib.rula_info_struct(info["RULA"]), None, out.data_ptr(), stream), "pr_rula_rows")
        assert np.array_equal(out.cpu().numpy(), plain_rula)
        got = ops.reba(eul, info["REBA"], rows=act).cpu().numpy()
        for a in np.unique(act):
            rows = act == a
            raised = dict(info["REBA"], Activity_Score=info["REBA"]["Activity_Score"] + int(a))
            assert np.array_equal(got[rows], reba_ref.reba_packed(pose[rows], raised)), ("reba", int(a))
        got = ops.rula(eul, info["RULA"], rows=torch.from_numpy(mus).to(gpu_device)).cpu().numpy()
        for m in np.unique(mus, axis=0):
            rows = (mus == m).all(axis=1)
            raised = dict(info["RULA"], A_Muscle_use_L=info["RULA"]["A_Muscle_use_L"] + int(m[0]),
                          A_Muscle_use_R=info["RULA"]["A_Muscle_use_R"] + int(m[1]), B_Muscle_use=info["RULA"]["B_Muscle_use"] + int(m[2]))
            assert np.array_equal(got[rows], rula_ref.rula_packed(pose[rows], raised)), ("rula", m.tolist())
    with pytest.raises(ValueError, match="rows"):
        ops.reba(eul, info["REBA"], rows=np.zeros(N + 1, np.int32))
    with pytest.raises(ValueError, match="rows"):
        ops.rula(eul, info["RULA"], rows=np.zeros((N, 3), np.float32))


# ---- the Predictor -----------------------------------------------------------------------------------------------------------------
N_FRAMES, FPS = 30, 10.0
KNOBS = dict(hold_seconds=1.0, rapid_seconds=0.3, gap_seconds=0.2)       # 10, 3 and 2 frames at 10 fps
STILL = (8, 24)                                                          # frames 8 .. 23 of the clip are one picture


@pytest.fixture(scope="module")
def clip():
    """30 frames of 160 x 120, noise except for a stretch of 16 identical ones, and two tracks with a fixed box each: under a
    fixed box identical frames are identical crops, hence identical rotations -- a planted still stretch."""
    rng = np.random.default_rng(9)
    frames = rng.integers(0, 256, (N_FRAMES, 120, 160, 3), dtype=np.uint8)
    frames[STILL[0]:STILL[1]] = frames[STILL[0]]
    tr = {5: {'bbox': np.tile(np.array([60, 60, 50, 100], np.float32), (N_FRAMES, 1)), 'frames': np.arange(N_FRAMES)},
          2: {'bbox': np.tile(np.array([110, 60, 40, 80], np.float32), (20, 1)), 'frames': np.r_[3:23]}}
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


@pytest.fixture()
def short_hold(monkeypatch):
    from poserisk_release_amd import dropin
    dropin.install()
    from core.config import cfg
    for k, v in KNOBS.items():
        monkeypatch.setitem(cfg.ACTIVITY, k, v)


@pytest.fixture(scope="module")
def knob_off(gpu_device, clip):
    frames, tr = clip
    return _predictor(gpu_device).score_people(frames, tr, synth.EXAMPLE_INFO, with_smpl_params=True)


def _same(a, b, what):
    assert list(a) == list(b), (what, list(a), list(b))
    for k in a:
        if k in ("reba", "rula"):
            (fa, sa, la, aa), (fb, sb, lb, ab) = a[k], b[k]
            assert np.array_equal(np.array(fa), np.array(fb), equal_nan=True) and np.array_equal(sa, sb) and np.array_equal(la, lb) and aa == ab, (what, k)
        elif k == "add_info":
            assert a[k] == b[k]
        else:
            assert np.asarray(a[k]).dtype == np.asarray(b[k]).dtype and np.array_equal(a[k], b[k]), (what, k)


def test_with_the_knob_off_every_array_and_file_is_todays(gpu_device, clip, knob_off, short_hold, tmp_path, monkeypatch):
    frames, tr = clip
    off = _predictor(gpu_device, derive_activity=False)
    again = off.score_people(frames, tr, synth.EXAMPLE_INFO, with_smpl_params=True, fps=FPS)
    assert again["ids"] == knob_off["ids"] == [5, 2]
    for a, b in zip(again["people"], knob_off["people"]):
        _same(a, b, "knob off")
        assert "activity" not in a
    target = off.score_frames(frames, tr, synth.EXAMPLE_INFO, with_smpl_params=True)
    _same(target, knob_off["people"][0], "the target")
    monkeypatch.setitem(sys.modules, "cv2", None)
    off.visualize = False
    off.persons = "all"
    off(str(tmp_path), "", str(tmp_path / "off"), frames=frames, tracking_results=tr, fps=FPS)
    names = sorted(os.listdir(tmp_path / "off"))
    assert "activity.json" not in names and "people.json" in names and "reba_result.txt" in names


def test_the_knob_raises_reba_by_the_derived_activity_and_rula_through_table_c(gpu_device, clip, knob_off, short_hold, tmp_path, monkeypatch):
    frames, tr = clip
    pred = _predictor(gpu_device, derive_activity=True, persons="all")
    people = pred.score_people(frames, tr, synth.EXAMPLE_INFO, with_smpl_params=True, fps=FPS)
    assert people["ids"] == [5, 2]
    info = synth.EXAMPLE_INFO
    for pid, out, raw in zip(people["ids"], people["people"], knob_off["people"]):
        n = len(raw["frames"])
        for k in ("result", "joint_cam", "debug_result", "rotmat", "betas", "cam", "frames", "bboxes"):      # the poses are the knob-off ones
            assert np.array_equal(out[k], raw[k]), (pid, k)
        par = out["activity"]["parameters"]
        assert (par["hold_frames"], par["rapid_frames"], par["gap_frames"], par["rep_events"], par["fps"]) == (10, 3, 2, 8, FPS)
        # this person's rotations alone, through the reference: the bits the shared call gave (score_people splits per person)
        ref = activity_ref.activity(raw["rotmat"], raw["frames"], [0, n], par["hold_frames"], par["rapid_frames"], par["gap_frames"],
                                    par["rep_events"], par["dot_static"], par["dot_move"], par["dot_rapid"])
        assert np.array_equal(out["activity"]["flags"], ref["flags"]) and np.array_equal(out["activity"]["adds"], ref["adds"])
        adds = ref["adds"]
        still = (np.asarray(raw["frames"]) >= STILL[0]) & (np.asarray(raw["frames"]) < STILL[1])
        assert (ref["flags"][still, 0] == 0xfff).all() and (adds[still, 0] >= 1).all() and (adds[still, 1:] == 1).all()      # the planted stretch
        # REBA: table C's value plus the activity score, so exactly the derived addend more than with the knob off
        assert np.array_equal(out["reba"][1], raw["reba"][1] + adds[:, 0]) and out["reba"][1][still].min() > raw["reba"][1][still].min()
        # RULA: muscle use enters before table C, so the oracle with the constants raised row by row says what comes out
        want = np.zeros(n, np.int64)
        for m in np.unique(adds[:, 1:], axis=0):
            rows = (adds[:, 1:] == m).all(axis=1)
            raised = dict(info["RULA"], A_Muscle_use_L=info["RULA"]["A_Muscle_use_L"] + int(m[0]),
                          A_Muscle_use_R=info["RULA"]["A_Muscle_use_R"] + int(m[1]), B_Muscle_use=info["RULA"]["B_Muscle_use"] + int(m[2]))
            want[rows] = rula_ref.rula_packed(raw["result"][rows], raised)[:, 0]
        assert np.array_equal(out["rula"][1], want) and (want >= raw["rula"][1]).all()
    # score_frames takes the same path: the target is element 0
    target = _predictor(gpu_device, derive_activity=True).score_frames(frames, tr, synth.EXAMPLE_INFO, with_smpl_params=True, fps=FPS)
    _same({k: v for k, v in target.items() if k != "activity"}, {k: v for k, v in people["people"][0].items() if k != "activity"}, "the target")
    assert np.array_equal(target["activity"]["adds"], people["people"][0]["activity"]["adds"])
    with pytest.raises(ValueError, match="fps"):
        pred.score_people(frames, tr, synth.EXAMPLE_INFO)
    # with smoothing on, the activity is that of the smoothed rotations
    both = _predictor(gpu_device, "REBA", derive_activity=True, smooth_median_radius=1, smooth_sigma=1.0)
    sm = both.score_frames(frames, tr, synth.EXAMPLE_INFO, with_smpl_params=True, fps=FPS)
    assert not np.array_equal(sm["rotmat"], knob_off["people"][0]["rotmat"])
    par = sm["activity"]["parameters"]
    ref = activity_ref.activity(sm["rotmat"], sm["frames"], [0, N_FRAMES], par["hold_frames"], par["rapid_frames"], par["gap_frames"],
                                par["rep_events"], par["dot_static"], par["dot_move"], par["dot_rapid"])
    assert np.array_equal(sm["activity"]["flags"], ref["flags"])
    # __call__ passes its fps and writes activity.json, which says what the arrays say
    monkeypatch.setitem(sys.modules, "cv2", None)
    pred.visualize = False
    ret = pred(str(tmp_path), "", str(tmp_path / "on"), frames=frames, tracking_results=tr, fps=FPS)
    doc = json.loads((tmp_path / "on" / "activity.json").read_text())
    assert doc["parameters"]["hold_seconds"] == 1.0 and doc["parameters"]["hold_frames"] == 10 and doc["joints"] == list(activity.JOINT_NAMES)
    assert [p["id"] for p in doc["people"]] == [5, 2]
    for entry, out in zip(doc["people"], ret["people"]["people"]):
        assert {k: entry[k] for k in activity.KINDS} == activity.counts(out["activity"]["flags"]) and entry["n_frames"] == len(out["frames"])
        assert entry["adds"] == {name: int(out["activity"]["adds"][:, c].sum()) for c, name in enumerate(activity.ADDS)}
        assert entry["held"]["rows"] >= STILL[1] - STILL[0] - 1
    assert np.array_equal(ret["people"]["people"][1]["activity"]["adds"], people["people"][1]["activity"]["adds"])


def test_two_ranks_derive_the_same_activity(gpu_device):
    """Two ranks sharing the GPU each score a shard, gather once and derive the activity of the same gathered rows: every rank
    ends with the single process' results, bit for bit (tests/activity_ranks_child.py)."""
    port = str(37500 + os.getpid() % 2000)
    child = os.path.join(REPO, "tests", "activity_ranks_child.py")
    procs = [subprocess.Popen([sys.executable, child, REPO, port, str(r)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
             for r in range(2)]
    outs = [p.communicate(timeout=600)[0] for p in procs]
    for p, o in zip(procs, outs):
        assert p.returncode == 0 and "ok" in o, o[-3000:]
