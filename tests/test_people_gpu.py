"""GPU: the people compositor (csrc/compose.hip, pr_compose_people) against pr_compose_video (the reduction property) and
against the numpy restatement of its contract (tests/video_people_ref.py), every byte; its tensors between guard bands; and
Predictor.score_people / Predictor.__call__ with persons='all' against score_frames and a persons='target' run."""
import ctypes as C
import json
import pickle
import sys
import types

import numpy as np
import pytest
import torch

import guard_band as gb
import people_cases as pc
import video_ref as vr
from poserisk_release_amd import _lib, synth, video

pytestmark = pytest.mark.gpu

_size_id = lambda s: "%dx%d_to_%dx%d_p%d" % s
_shape_id = lambda s: "K%d_L%d_Limg%d" % s


def _atlas_dev(c, dev):
    a = c["atlas"]
    return (torch.from_numpy(np.array(a.cov)).to(dev), a.adv, a.ascent)


def _run(c, dev, **kw):
    out, st = video.compose_people(torch.from_numpy(c["frames"]).to(dev), c["src_idx"], c["box"], c["box_rgb"], c["lines"], c["text"],
                                   c["L_img"], _atlas_dev(c, dev), c["dst_h"], c["dst_w"], c["panel_w"], return_status=True, **kw)
    return out.cpu().numpy(), st.cpu().numpy()


# ---- reduction: K = 1, L_img = 0 is pr_compose_video ----------------------------------------------------------------------------
@pytest.mark.parametrize("size", pc.SIZES, ids=_size_id)
def test_one_box_and_no_tags_is_pr_compose_video_byte_for_byte(gpu_device, size):
    c = pc.case(size, (1, 16, 0), seed=21, N=3, reduction=True)
    c["box_rgb"][:] = c["box_rgb"][0, 0]                                  # pr_compose_video has one colour a call
    got, st = _run(c, gpu_device)
    want, want_st = video.compose(torch.from_numpy(c["frames"]).to(gpu_device), c["src_idx"], c["box"][:, 0], c["lines"], c["text"],
                                  _atlas_dev(c, gpu_device), c["dst_h"], c["dst_w"], c["panel_w"], box_rgb=tuple(c["box_rgb"][0, 0, :3]),
                                  return_status=True)
    assert got.shape == (3, size[3], size[2] + size[4], 3)
    assert np.array_equal(got, want.cpu().numpy()) and np.array_equal(st, want_st.cpu().numpy()) and st.tolist() == [0, 0, 0]
    assert got[:, :, :size[2]].any() and got[:, :, size[2]:].any()
    # one kernel serves both entry points, so both are also held against the numpy restatement of pr_compose_video's contract
    a = c["atlas"]
    ref, ref_st = vr.compose(c["frames"], c["src_idx"], c["box"][:, 0], c["lines"], c["text"], np.asarray(a.cov), a.adv, a.ascent,
                             c["dst_h"], c["dst_w"], c["panel_w"], c["box_rgb"][0, 0, :3])
    assert np.array_equal(got, ref) and np.array_equal(want.cpu().numpy(), ref) and ref_st.tolist() == [0, 0, 0]


# ---- the contract, every byte ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", pc.SHAPES, ids=_shape_id)
@pytest.mark.parametrize("size", pc.SIZES, ids=_size_id)
def test_compose_people_matches_the_reference_bit_for_bit(gpu_device, size, shape):
    """people_cases.case places: two overlapping boxes in different colours, a box wholly off the frame, x_max < x_min in a middle
    slot, boxes across every frame edge; tags that start left of x = 0, run across the image / panel boundary, overlap each
    other and sit on a box outline; L_img = 0, L_img = L and L = 32; a src_idx outside the range in the last canvas."""
    c = pc.case(size, shape, seed=sum(size) + sum(shape))
    got, st = _run(c, gpu_device)
    want, want_st = pc.reference(c)
    assert np.array_equal(st, want_st) and st.tolist() == [0, 0, 0, 1]
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"{len(bad)} bytes differ, first (canvas, row, col, channel) {bad[0].tolist()}"
    dst_w = size[2]
    # the canvas without a frame: a zero image region under the tags, the panel drawn all the same
    no_lines, _ = pc.reference(dict(c, lines=None, text=None), [3])
    assert not no_lines[3].any()
    if shape[2] < shape[1]:
        assert got[3, :, dst_w:].any()
    if shape[2] > 0:
        assert got[3, :, :dst_w].any() and (got[0, :, :dst_w] != pc.reference(dict(c, lines=None, text=None), [0])[0][0, :, :dst_w]).any()


def test_no_canvases_and_every_argument_error(gpu_device):
    lib = _lib.load()
    c = pc.case(pc.SIZES[0], (2, 8, 3), seed=4)
    W, H, dst_w, dst_h, panel_w = pc.SIZES[0]
    a = c["atlas"]
    t = {k: torch.from_numpy(np.ascontiguousarray(c[k])).to(gpu_device) for k in ("frames", "src_idx", "box", "box_rgb", "lines", "text")}
    cov = torch.from_numpy(np.array(a.cov)).to(gpu_device)
    out = torch.full((4, dst_h, dst_w + panel_w, 3), 7, dtype=torch.uint8, device=gpu_device)
    status = torch.full((4,), -7, dtype=torch.int32, device=gpu_device)
    stream = torch.cuda.current_stream().cuda_stream
    pad = lambda v: (C.c_int * 4)(*(list(v) + [0] * (4 - len(v))))

    def call(**over):
        v = dict(frames=t["frames"].data_ptr(), src_idx=t["src_idx"].data_ptr(), box=t["box"].data_ptr(), box_rgb=t["box_rgb"].data_ptr(),
                 lines=t["lines"].data_ptr(), text=t["text"].data_ptr(), atlas=cov.data_ptr(), out=out.data_ptr(), status=status.data_ptr(),
                 N=4, n_frames=3, H=H, W=W, dst_h=dst_h, dst_w=dst_w, panel_w=panel_w, K=2, L=8, L_img=3, C=9, S=3, CH=11, CW=7,
                 adv=pad(a.adv), ascent=pad(a.ascent))
        v.update(over)
        rc = lib.pr_compose_people(C.byref(_lib.ComposePeopleArgs(**v)), stream)
        return rc, lib.pr_last_error().decode()
    for over, word in ((dict(N=-1), "N = -1"), (dict(out=None), "null out"), (dict(frames=None), "null frames"), (dict(n_frames=0), "n_frames"),
                       (dict(H=0), "1..4096"), (dict(W=4097), "1..4096"), (dict(dst_w=0), "dst_w"), (dict(dst_h=4097), "dst_h"),
                       (dict(panel_w=-1), "panel_w"), (dict(K=0), "K = 0"), (dict(K=17), "K = 17"), (dict(box_rgb=None), "box_rgb"),
                       (dict(L=33), "L = 33"), (dict(L_img=-1), "L_img = -1"), (dict(L_img=9), "L_img = 9"), (dict(lines=None), "null lines"),
                       (dict(text=None), "null lines"), (dict(atlas=None), "null lines"), (dict(C=0), "C = 0"), (dict(S=5), "S = 5"),
                       (dict(CH=257), "CH x CW"), (dict(adv=pad((0, 5, 3))), "adv[0]"), (dict(ascent=pad((9, 5000, 0))), "ascent[1]"),
                       (dict(src_idx=None), "without src_idx")):
        rc, msg = call(**over)
        assert rc == -1 and word in msg and "pr_compose_people" in msg, (over, rc, msg)       # PR_ERR_INVALID
    assert lib.pr_compose_people(None, stream) == -1
    assert call(N=0, out=None, frames=None)[0] == 0                     # N = 0: PR_OK, nothing looked at
    torch.cuda.synchronize()
    assert (out == 7).all() and (status == -7).all()                    # no device work happened
    assert call()[0] == 0                                               # and the call these were derived from is valid
    torch.cuda.synchronize()
    want, want_st = pc.reference(c)
    assert np.array_equal(out.cpu().numpy(), want) and status.cpu().tolist() == want_st.tolist()
    with pytest.raises(ValueError, match="come together"):
        video.compose_people(t["frames"], c["src_idx"], c["box"])
    with pytest.raises(ValueError, match="box_rgb must have shape"):
        video.compose_people(t["frames"], c["src_idx"], c["box"], c["box_rgb"][:, :1])
    with pytest.raises(_lib.PoseRiskHipError, match="CUDA tensor"):
        video.compose_people(c["frames"], c["src_idx"], c["box"], c["box_rgb"])


# ---- guard bands ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size,shape", [(pc.SIZES[0], pc.SHAPES[2]), (pc.SIZES[1], pc.SHAPES[1]), (pc.SIZES[2], pc.SHAPES[0])],
                         ids=lambda v: _size_id(v) if len(v) == 5 else _shape_id(v))
def test_every_tensor_stays_inside_its_guard_bands(gpu_device, size, shape):
    """The output and the status between canary guards, every input between guards of 255 / 0x7fffffff (tests/guard_band.py): a
    read outside a tensor that reaches an output changes a byte the reference has, a store outside one lands in a guard."""
    c = pc.case(size, shape, seed=77)
    a = c["atlas"]
    W, H, dst_w, dst_h, panel_w = size
    K, L, L_img = shape
    N = len(c["src_idx"])
    ins = {k: torch.from_numpy(np.ascontiguousarray(c[k])).to(gpu_device) for k in ("frames", "src_idx", "box", "box_rgb", "lines", "text")}
    ins["cov"] = torch.from_numpy(np.array(a.cov)).to(gpu_device)
    pad = lambda v: (C.c_int * 4)(*(list(v) + [0] * (4 - len(v))))

    def call(i, o):
        args = _lib.ComposePeopleArgs(i["frames"].data_ptr(), i["src_idx"].data_ptr(), i["box"].data_ptr(), i["box_rgb"].data_ptr(),
                                      i["lines"].data_ptr(), i["text"].data_ptr(), i["cov"].data_ptr(), o["out"].data_ptr(),
                                      o["status"].data_ptr(), N, 3, H, W, dst_h, dst_w, panel_w, K, L, L_img, c["text"].shape[2],
                                      a.cov.shape[0], a.cov.shape[2], a.cov.shape[3], pad(a.adv), pad(a.ascent))
        _lib.check(_lib.load().pr_compose_people(C.byref(args), torch.cuda.current_stream().cuda_stream), "pr_compose_people")
    # a canvas byte may be 0x5A in its own right: the comparison below says whether every byte was written
    got = gb.run_guarded(call, ins, {"out": ((N, dst_h, dst_w + panel_w, 3), torch.uint8), "status": ((N,), torch.int32)},
                         may_hold_canary=("out",))
    want, want_st = pc.reference(c)
    assert np.array_equal(got["out"].cpu().numpy(), want) and got["status"].cpu().tolist() == want_st.tolist()


# ---- the Predictor: batching changes nothing, and the persons knob end to end -------------------------------------------------------
N_FRAMES = 24


@pytest.fixture(scope="module")
def clip():
    """24 frames of 160 x 120 and three tracks of 24, 17 and 9 frames, largest box first: at batch 16 the 50 rows straddle both
    person boundaries (rows 24 and 41)."""
    rng = np.random.default_rng(9)
    frames = rng.integers(0, 256, (N_FRAMES, 120, 160, 3), dtype=np.uint8)
    tr = {}
    for pid, (first, n, w, h, x) in {5: (0, 24, 50, 100, 40), 2: (4, 17, 40, 80, 90), 11: (15, 9, 30, 60, 130)}.items():
        tr[pid] = {'bbox': np.stack([np.array([x + i, 60 - i % 3, w, h], np.float32) for i in range(n)]), 'frames': np.arange(first, first + n)}
    return frames, tr


def _predictor(gpu_device, score_type="REBA,RULA", debug=False, **knobs):
    from poserisk_release_amd import dropin
    dropin.install()
    from core import base
    from models import hmr
    from smpl import SMPL
    model = hmr()
    model.load_state_dict(synth.hmr_state_dict(seed=1), strict=False)
    smpl = SMPL(models={"neutral": synth.smpl_model(V=6890, seed=2)}, device=gpu_device)
    args = types.SimpleNamespace(gpu="0", type=score_type, debug=debug, debug_joints="", debug_frame=-1, **knobs)
    return base.Predictor(args, spin_model=model, smpl_model=smpl, batch_size=16)


def _same(a, b, what):
    assert list(a) == list(b), (what, list(a), list(b))
    for k in a:
        if k in ("reba", "rula"):
            (fa, sa, la, aa), (fb, sb, lb, ab) = a[k], b[k]
            assert np.array_equal(np.array(fa), np.array(fb), equal_nan=True) and np.array_equal(sa, sb) and np.array_equal(la, lb) and aa == ab, (what, k)
        else:
            assert np.asarray(a[k]).dtype == np.asarray(b[k]).dtype and np.array_equal(a[k], b[k]), (what, k)


def test_people_share_batches_and_keep_their_bits(gpu_device, clip, monkeypatch):
    from poserisk_release_amd import ops
    frames, tr = clip
    pred = _predictor(gpu_device)
    launches = []
    real = ops.crop_frames
    monkeypatch.setattr(ops, "crop_frames", lambda *a, **k: (launches.append(len(a[1])), real(*a, **k))[1])
    people = pred.score_people(frames, tr, synth.EXAMPLE_INFO)
    assert launches == [16, 16, 16, 2]                                   # 50 rows in 4 launches; one person at a time: 2 + 2 + 1
    assert people["ids"] == [5, 2, 11] and people["frames_total"] == N_FRAMES and set(people) == {"people", "ids", "frames_total"}
    for p, pid in enumerate(people["ids"]):
        alone = pred.score_frames(frames, {pid: tr[pid]}, synth.EXAMPLE_INFO)
        _same(people["people"][p], alone, f"person {pid}")
    _same(people["people"][0], pred.score_frames(frames, tr, synth.EXAMPLE_INFO), "the target")
    # the same range check and message as score_frames
    off = dict(tr)
    off[2] = dict(tr[2], frames=tr[2]['frames'] + 10)
    with pytest.raises(ValueError, match=r"name frames 0\.\.30 but only 24 frames were decoded"):
        pred.score_people(frames, off, synth.EXAMPLE_INFO)
    with pytest.raises(NotImplementedError, match="render_mesh"):
        _predictor(gpu_device, render_mesh=True).score_people(frames, tr, synth.EXAMPLE_INFO)
    from poserisk_release_amd import pipeline as pl
    monkeypatch.setattr(pl, "world_and_rank", lambda: (2, 0))
    with pytest.raises(NotImplementedError, match="world_size"):
        pred.score_people(frames, tr, synth.EXAMPLE_INFO)


def test_with_debug_every_person_gets_its_own_rows_of_the_angle_logs(gpu_device, clip):
    frames, tr = clip
    people = _predictor(gpu_device, debug=True).score_people(frames, tr, synth.EXAMPLE_INFO)
    assert list(people) == ["people", "ids", "frames_total", "pose_logs"] and len(people["pose_logs"]) == 3
    for p, pid in enumerate(people["ids"]):
        alone = _predictor(gpu_device, debug=True)                      # fresh: its scorers' logs start empty
        alone.score_frames(frames, {pid: tr[pid]}, synth.EXAMPLE_INFO)
        assert list(people["pose_logs"][p]) == ["reba", "rula"]
        for key, scorer in (("reba", alone.reba), ("rula", alone.rula)):
            assert len(scorer.log) == len(tr[pid]['frames']) and people["pose_logs"][p][key] == scorer.log, (pid, key)
    assert people["pose_logs"][1]["reba"][0] != people["pose_logs"][0]["reba"][0]


def test_persons_all_end_to_end(gpu_device, clip, tmp_path, monkeypatch):
    from PIL import Image
    monkeypatch.setitem(sys.modules, "cv2", None)                      # with or without cv2 the files are the GPU's
    frames, tr = clip
    src = tmp_path / "clip"
    src.mkdir()
    np.save(src / "frames.npy", frames)
    with open(src / "tracking.pkl", "wb") as f:
        pickle.dump(tr, f)
    with pytest.raises(ValueError, match="everyone"):
        _predictor(gpu_device, persons="everyone")
    pred = _predictor(gpu_device, "REBA", gpu_video=True, video_codec="png", persons="all")
    monkeypatch.setattr(type(pred), "score_frames", lambda self, *a, **k: pytest.fail("persons='all' runs the model once"))
    out = pred(str(src), "", str(tmp_path / "all"))
    monkeypatch.undo()
    monkeypatch.setitem(sys.modules, "cv2", None)
    one = _predictor(gpu_device, "REBA", gpu_video=True, video_codec="png")(str(src), "", str(tmp_path / "one"))
    assert "people" not in one and not (tmp_path / "one" / "people.json").exists()
    # every top-level file is what a persons='target' run writes
    top = sorted(p.relative_to(tmp_path / "one") for p in (tmp_path / "one").rglob("*") if p.is_file())
    assert len(top) == 2 + N_FRAMES and all((tmp_path / "all" / p).read_bytes() == (tmp_path / "one" / p).read_bytes() for p in top)
    extra = sorted(str(p.relative_to(tmp_path / "all")) for p in (tmp_path / "all").rglob("*") if p.is_file() and p.relative_to(tmp_path / "all") not in top)
    assert extra == sorted(["people.json"] + [f"person_{i}/{f}" for i in (5, 2, 11) for f in ("REBA_score.png", "reba_result.txt")] +
                           ["REBA_people/{0:09d}.png".format(i) for i in range(N_FRAMES)])
    people = out["people"]
    assert people["ids"] == [5, 2, 11]
    assert (tmp_path / "all" / "person_5" / "reba_result.txt").read_bytes() == (tmp_path / "all" / "reba_result.txt").read_bytes()
    doc = json.loads((tmp_path / "all" / "people.json").read_text())
    assert doc["frames_total"] == N_FRAMES and [p["id"] for p in doc["people"]] == [5, 2, 11]
    for entry, o in zip(doc["people"], people["people"]):
        final, _, _, (level, name) = o["reba"]
        assert (entry["first_frame"], entry["last_frame"], entry["n_frames"]) == (int(o["frames"][0]), int(o["frames"][-1]), len(o["frames"]))
        assert entry["mean_box_area"] == float((o["bboxes"][:, 2] * o["bboxes"][:, 3]).mean())
        assert [entry["REBA"][k] for k in ("avg", "top50", "top10", "max", "mode")] == [None if np.isnan(v) else float(v) for v in final]
        assert entry["REBA"]["action_level"] == level and entry["REBA"]["action"] == name and "RULA" not in entry
        txt = (tmp_path / "all" / f"person_{entry['id']}" / "reba_result.txt").read_text()
        assert txt.startswith(f"AVG Score: {final[0]} ") and f"Action level: {level} " in txt
    # frame 5 of the people video is the reference composer's canvas of what people_draw_list says
    ppl = []
    for pid, o in zip(people["ids"], people["people"]):
        acts = [pred.reba.action_level(s) for s in o["reba"][1]]
        ppl.append(dict(id=pid, frames=o["frames"], bboxes=o["bboxes"], scores=o["reba"][1], levels=[a[0] for a in acts], names=[a[1] for a in acts]))
    dst_h, dst_w, panel_w = video.canvas_size(120, 160)
    draw = video.people_draw_list("REBA", N_FRAMES, ppl, dst_h, dst_w, 120, 160)
    assert draw.box.shape[1] == 3 and len(draw.tags[5]) == 2 and len(draw.tags[20]) == 3      # frame 5 shows two of the three
    lines, codes, L_img = video.pack_people(draw, 0, N_FRAMES, C=max(len(s[0]) for g in (draw.tags, draw.panel) for t in g for s in t))
    atlas = video.font_atlas()
    import video_people_ref as pref
    want, _ = pref.compose_people(frames, np.arange(N_FRAMES), draw.box, draw.box_rgb, lines, codes, L_img, np.asarray(atlas.cov), atlas.adv,
                                  atlas.ascent, dst_h, dst_w, panel_w, canvases=[5])
    got = np.asarray(Image.open(tmp_path / "all" / "REBA_people" / "000000005.png").convert("RGB"))
    assert got.shape == (dst_h, dst_w + panel_w, 3) and np.array_equal(got, want[5])
    assert want[5][:, :dst_w].any() and want[5][:, dst_w:].any()
