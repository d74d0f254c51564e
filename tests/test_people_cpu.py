"""CPU: the host half of scoring every tracked person -- tracks.people_tracks, video.people_draw_list, the numpy restatement of
the people contract (tests/video_people_ref.py) against pr_compose_video's restatement, the ABI surface of pr_compose_people,
and what Predictor.__call__ does with the persons knob unset and set (the model stubbed out)."""
import ctypes as C
import json
import os
import re
import types

import numpy as np
import pytest

import people_cases as pc
import video_ref as vr
from conftest import REPO
from poserisk_release_amd import _lib, dropin, render, tracks, video

dropin.install()
from core import base  # noqa: E402
from core.config import cfg  # noqa: E402
from reba import REBA  # noqa: E402
from rula import RULA  # noqa: E402


def _track(n, w, h, first=0):
    return {'bbox': np.tile(np.array([50, 40, w, h], np.float32), (n, 1)), 'frames': np.arange(first, first + n)}


# ---- tracks.people_tracks ---------------------------------------------------------------------------------------------------
def test_people_tracks_order_ties_and_fallback():
    tr = {7: _track(40, 10, 10), 3: _track(50, 30, 20), 9: _track(60, 20, 30), 4: _track(10, 99, 99), 5: _track(34, 5, 5)}
    got = tracks.people_tracks(tr, 100, 0.33)
    # 4 has too few frames (10 < 33); 3 and 9 tie at 600 and keep the dict's order; then 7 (100), 5 (25)
    assert [g[0] for g in got] == [3, 9, 7, 5]
    assert got[0][1].dtype == np.float32 and got[0][1].shape == (50, 4) and got[0][2].tolist() == list(range(50))
    # no track qualifies: all are kept, the short one with the large box first
    assert [g[0] for g in tracks.people_tracks(tr, 1000, 0.33)] == [4, 3, 9, 7, 5]
    # the 1000-frame cap: 0.33 * 4000 = 1320 frames asked for, 1000 are enough
    long = {1: _track(1000, 5, 5), 2: _track(999, 50, 50)}
    assert [g[0] for g in tracks.people_tracks(long, 4000, 0.33)] == [1]
    assert tracks.people_tracks({}, 10) == []


def test_people_tracks_element_0_is_the_target_track():
    rng = np.random.default_rng(0)
    for trial in range(200):
        n_frames = int(rng.integers(5, 60))
        tr = {}
        for pid in rng.permutation(12)[:int(rng.integers(1, 7))]:
            n = int(rng.integers(1, n_frames + 1))
            box = rng.uniform(1, 80, (n, 4)).astype(np.float32)
            if rng.random() < 0.3:
                box[:, 2:] = 8.0                                    # equal areas: the tie rule decides
            tr[int(pid)] = {'bbox': box, 'frames': np.sort(rng.permutation(n_frames)[:n])}
        ratio = float(rng.choice([0.0, 0.33, 0.9]))
        box, frames = tracks.target_track(tr, n_frames, ratio)
        got = tracks.people_tracks(tr, n_frames, ratio)
        assert np.array_equal(got[0][1], box) and np.array_equal(got[0][2], frames), trial
        assert len({g[0] for g in got}) == len(got) == len(tracks.filter_tracks(tr, n_frames, ratio))
        area = [(g[1][:, 2] * g[1][:, 3]).mean() for g in got]
        assert all(a >= b for a, b in zip(area, area[1:]))


# ---- video.people_draw_list -------------------------------------------------------------------------------------------------
def _person(pid, frames, boxes, scores, scorer):
    acts = [scorer.action_level(s) for s in scores]
    return dict(id=pid, frames=np.array(frames), bboxes=np.array(boxes, np.float32), scores=np.array(scores),
                levels=[a[0] for a in acts], names=[a[1] for a in acts])


def test_people_draw_list_every_field_of_a_three_person_case():
    assert np.array_equal(np.array(video.PEOPLE_LEVEL_RGB[:4], np.uint8), render.LEVEL_RGB) and len(video.PEOPLE_LEVEL_RGB) == 5
    H, W, dst_w = 200, 400, 720
    canvas_h = video.canvas_size(H, W)[0]                                 # 360
    r = REBA()
    people = [_person(4, [0, 1, 2], [[200, 100, 100, 80]] * 3, [1, 5, 11], r),        # tag above the box
              _person(9, [1, 2], [[60, 20, 41, 39]] * 2, [3, 8], r),                  # at the top edge: the tag flips below
              _person(2, [2], [[-10, 150, 30, 30]], [2], r)]                          # across the left edge, absent from 0 and 1
    d = video.people_draw_list("REBA", 4, people, canvas_h, dst_w, H, W)
    assert d.box.shape == (4, 3, 4) and d.box.dtype == np.int32 and d.box_rgb.shape == (4, 3, 4) and d.box_rgb.dtype == np.uint8
    no = list(video.NO_BOX)
    assert d.box[0].tolist() == [[150, 60, 250, 140], no, no]
    assert d.box[1].tolist() == [[150, 60, 250, 140], [40, 1, 80, 39], no]
    assert d.box[2].tolist() == [[150, 60, 250, 140], [40, 1, 80, 39], [-25, 135, 5, 165]]
    assert d.box[3].tolist() == [no, no, no]
    rgb = video.PEOPLE_LEVEL_RGB
    assert d.box_rgb[2, :, :3].tolist() == [list(rgb[4]), list(rgb[3]), list(rgb[1])]       # 11: level 5, 8: level 4, 2: level 2
    assert d.box_rgb[0, 0, :3].tolist() == list(rgb[0]) and d.box_rgb[1, 0, :3].tolist() == list(rgb[2]) and not d.box_rgb[..., 3].any()
    # tags: origin = the box's top-left corner on the canvas (x 720 / 400, y 360 / 200, floored), baseline 3 px above it ...
    assert d.tags[0] == [("#4 1", (270, 108 - 3), 0, rgb[0])]
    # ... or, where fewer than TAG_H rows are left above (y = 1 -> row 1), TAG_GAP + TAG_H below the corner
    assert d.tags[1] == [("#4 5", (270, 105), 0, rgb[2]), ("#9 3", (72, 1 + video.TAG_GAP + video.TAG_H), 0, rgb[1])]
    assert d.tags[2][2] == ("#2 2", (-25 * 720 // 400, 135 * 360 // 200 - 3), 0, rgb[1]) and (-25 * 720 // 400) == -45
    assert d.tags[3] == []
    # the panel: the header in the score colour, a line per person in people order, the frame line
    x = dst_w + 15
    assert d.panel[0] == [("REBA people: 1", (x, 35), 2, video.GREEN), ("#4  1  Negligible risk", (x, 70), 0, rgb[0]),
                          ("frame: 0", (x, canvas_h - 14), 0, video.WHITE)]
    assert d.panel[2][1:4] == [("#4  11  Very high risk. Implement change"[:video.PANEL_CHARS], (x, 70), 0, rgb[4]),
                               ("#9  8  High risk. Investigate and implement change"[:video.PANEL_CHARS], (x, 94), 0, rgb[3]),
                               ("#2  2  Low risk. Change may be needed."[:video.PANEL_CHARS], (x, 118), 0, rgb[1])]
    assert d.panel[3] == [("REBA people: 0", (x, 35), 2, video.GREEN), ("frame: 3", (x, canvas_h - 14), 0, video.WHITE)]
    # a frame shows its own score: frame 1 of person 4 is 5, not the even-index 1 draw_list would show
    assert d.tags[1][0][0] == "#4 5"
    # BGR frames: the colours swapped
    b = video.people_draw_list("REBA", 4, people, canvas_h, dst_w, H, W, bgr=True)
    assert b.box_rgb[2, 0, :3].tolist() == list(rgb[4][::-1]) and b.tags[0][0][3] == rgb[0][::-1]
    # and the whole thing packs into pr_compose_people's arrays: tags first, padded to K slots
    lines, codes, L_img = video.pack_people(d, 0, 4)
    assert L_img == 3 and lines.shape == (4, 3 + 5, 5) and lines[0, 1:3, 3].tolist() == [0, 0] and lines[0, 3, 3] == len("REBA people: 1")
    assert bytes(codes[2, 2, :4]) == b"#2 2"


def test_people_draw_list_17_people_draw_the_16_largest_and_list_14():
    u = RULA()
    people = [_person(i, [0], [[100 + 10 * i, 100, 20 + (i * 7) % 17, 30]], [1 + i % 7], u) for i in range(17)]
    widths = [20 + (i * 7) % 17 for i in range(17)]
    smallest = int(np.argmin(widths))                                    # widths are distinct mod 17: one smallest box
    assert sorted(widths)[0] != sorted(widths)[1]
    d = video.people_draw_list("RULA", 1, people, 450, 720, 450, 800)
    assert d.box.shape == (1, 16, 4) and len(d.tags[0]) == 16
    drawn = [int(t[0].split()[0][1:]) for t in d.tags[0]]
    assert drawn == [i for i in range(17) if i != smallest]                # still in people order
    assert d.panel[0][0][0] == "RULA people: 17" and len(d.panel[0]) == 1 + video.PEOPLE_PANEL_ROWS + 1
    assert [p[0].split()[0] for p in d.panel[0][1:-1]] == [f"#{i}" for i in drawn[:14]]
    lines, codes, L_img = video.pack_people(d, 0, 1)
    assert L_img == 16 and lines.shape[1] == 32 == video.PEOPLE_MAX_LINES


# ---- the restatement itself: the reduction property -----------------------------------------------------------------------------
@pytest.mark.parametrize("size", pc.SIZES, ids=lambda s: "%dx%d_to_%dx%d_p%d" % s)
def test_reference_composer_reduces_to_the_single_box_one(size):
    c = pc.case(size, (1, 16, 0), seed=11, N=4)                          # K = 1, L_img = 0, with a frame that does not exist
    a = c["atlas"]
    want, want_st = vr.compose(c["frames"], c["src_idx"], c["box"][:, 0], c["lines"], c["text"], np.asarray(a.cov), a.adv, a.ascent,
                               c["dst_h"], c["dst_w"], c["panel_w"], c["box_rgb"][0, 0, :3])
    c1 = dict(c, box_rgb=np.tile(c["box_rgb"][0:1, 0:1], (4, 1, 1)))      # one colour for every canvas, as pr_compose_video has
    got, st = pc.reference(c1)
    assert np.array_equal(got, want) and np.array_equal(st, want_st) and st.tolist() == [0, 0, 0, 1]
    assert got[:, :, :c["dst_w"]].any() and got[:, :, c["dst_w"]:].any()


def test_reference_composer_tags_stay_on_the_image_and_panel_lines_on_the_panel():
    c = pc.case(pc.SIZES[1], (5, 12, 12), seed=2)                         # tags only
    out, _ = pc.reference(c)
    plain, _ = pc.reference(dict(c, lines=None, text=None))
    assert not out[:, :, c["dst_w"]:].any() and (out[:, :, :c["dst_w"]] != plain[:, :, :c["dst_w"]]).any()
    c = pc.case(pc.SIZES[1], (2, 8, 0), seed=2)                           # panel lines only
    out, _ = pc.reference(c)
    plain, _ = pc.reference(dict(c, lines=None, text=None))
    assert np.array_equal(out[:, :, :c["dst_w"]], plain[:, :, :c["dst_w"]]) and out[:, :, c["dst_w"]:].any()
    # later boxes over earlier ones: swapping two overlapping slots changes pixels
    c = pc.case(pc.SIZES[1], (2, 8, 0), seed=2)
    swapped = dict(c, box=c["box"][:, ::-1], box_rgb=c["box_rgb"][:, ::-1])
    assert (pc.reference(c, [0])[0][0] != pc.reference(swapped, [0])[0][0]).any()


# ---- the ABI surface ----------------------------------------------------------------------------------------------------------
def test_header_binding_and_library_agree_on_pr_compose_people():
    hdr = open(os.path.join(REPO, "include", "poserisk_hip.h")).read()
    assert "/* r3 " in hdr and hdr.index("/* r2 ") < hdr.index("/* r3 ") < hdr.index("/* j1 ")
    assert re.search(r"\bint\s+pr_compose_people\s*\(\s*const\s+pr_compose_people_args\s*\*", hdr)
    assert re.search(r"#define\s+PR_PEOPLE_MAX_BOXES\s+16\b", hdr) and re.search(r"#define\s+PR_PEOPLE_MAX_LINES\s+32\b", hdr)
    assert (video.PEOPLE_MAX_BOXES, video.PEOPLE_MAX_LINES) == (16, 32)
    assert "pr_compose_people" in _lib.SIGNATURES
    lib = _lib.load()
    assert lib.pr_abi_version() == _lib.ABI_VERSION == 16
    assert hasattr(lib, "pr_compose_people")
    # 9 pointers, 14 ints, 2 x 4 ints
    assert C.sizeof(_lib.ComposePeopleArgs) == 9 * 8 + 14 * 4 + 32
    assert lib.pr_compose_people(None, None) == -1 and b"pr_compose_people" in lib.pr_last_error()
    args = _lib.ComposePeopleArgs()
    assert lib.pr_compose_people(C.byref(args), None) == 0                # N = 0: nothing to do


# ---- Predictor.__call__ and the knob ----------------------------------------------------------------------------------------------
def _canned(scorer_r, scorer_u, n, seed):
    rng = np.random.default_rng(seed)
    out = dict(result=rng.uniform(-90, 90, (n, 24, 3)), joint_cam=rng.standard_normal((n, 24, 3)).astype(np.float32),
               debug_result=rng.standard_normal((n, 24, 3)).astype(np.float32))
    for key, scorer, width in (("reba", scorer_r, 6), ("rula", scorer_u, 7)):
        scores = rng.integers(1, 8, n)
        final = base.aggregate(scores)
        out[key] = (final, scores, np.array([[str(v) for v in rng.integers(1, 4, width)] for _ in range(n)]), scorer.action_level(final[4]))
    out["frames"] = np.arange(2, 2 + n)
    out["bboxes"] = np.tile(np.array([30, 20, 10 + seed, 20], np.float32), (n, 1))
    return out


def _bare_predictor(**attrs):
    pred = object.__new__(base.Predictor)
    pred.__dict__.update(dict(debugging=False, debug_frame=-1, debug_joints=None, gpu_video=False, render_mesh=False, visualize=False,
                              reba=REBA(), rula=RULA(), run_reba=True, run_rula=True), **attrs)
    return pred


def _files(root):
    return sorted(os.path.relpath(os.path.join(d, f), root) for d, _, fs in os.walk(root) for f in fs)


def test_with_persons_unset_call_touches_nothing_new(tmp_path, monkeypatch):
    assert cfg.DATASET.persons == "target"
    pred = _bare_predictor()                                             # no `persons` attribute at all: the default
    target = _canned(pred.reba, pred.rula, 12, 1)

    def forbidden(*a, **k):
        raise AssertionError("persons='target' must not reach the people path")
    for name in ("score_people", "write_people_reports", "write_people_video"):
        monkeypatch.setattr(base.Predictor, name, forbidden)
    monkeypatch.setattr(base.Predictor, "score_frames", lambda self, *a, **k: dict(target))
    frames = np.zeros((20, 8, 8, 3), np.uint8)
    out = pred(None, None, str(tmp_path / "out"), frames=frames, tracking_results={1: None})
    assert "people" not in out and out["fps"] == 30.0
    assert _files(tmp_path / "out") == ["REBA_score.png", "RULA_score.png", "reba_result.txt", "rula_result.txt"]


def test_persons_all_adds_the_person_folders_and_people_json_and_leaves_the_rest(tmp_path, monkeypatch, capsys):
    pred = _bare_predictor(persons="all", visualize=True)                # visualize on, gpu_video off: the people video is skipped, by name
    outs = [_canned(pred.reba, pred.rula, n, s) for n, s in ((12, 1), (9, 2), (5, 3))]
    people = {"people": outs, "ids": [np.int64(8), 3, "left"], "frames_total": 20}
    monkeypatch.setattr(base.Predictor, "score_people", lambda self, *a, **k: people)
    monkeypatch.setattr(base.Predictor, "score_frames", lambda self, *a, **k: pytest.fail("the model must run once"))
    import poserisk_release_amd.reports as reports
    monkeypatch.setattr(reports, "write_annotated_video", lambda *a, **k: None)
    frames = np.zeros((20, 8, 8, 3), np.uint8)
    out = pred(None, None, str(tmp_path / "all"), frames=frames, tracking_results={1: None})
    assert "needs the gpu_video knob" in capsys.readouterr().out
    assert out["people"] is people and np.array_equal(out["result"], outs[0]["result"])
    per_person = ["REBA_score.png", "RULA_score.png", "reba_result.txt", "rula_result.txt"]
    assert _files(tmp_path / "all") == sorted(per_person + ["people.json"] + [f"person_{i}/{f}" for i in (8, 3, "left") for f in per_person])
    # the top level is the target's, byte for byte what a 'target' run writes
    monkeypatch.setattr(base.Predictor, "score_frames", lambda self, *a, **k: dict(outs[0]))
    _bare_predictor(visualize=True)(None, None, str(tmp_path / "one"), frames=frames, tracking_results={1: None})
    for f in per_person:
        assert (tmp_path / "all" / f).read_bytes() == (tmp_path / "one" / f).read_bytes(), f
        assert (tmp_path / "all" / "person_8" / f).read_bytes() == (tmp_path / "one" / f).read_bytes(), f
    assert (tmp_path / "all" / "person_3" / "reba_result.txt").read_text().startswith(f"AVG Score: {outs[1]['reba'][0][0]} ")
    doc = json.loads((tmp_path / "all" / "people.json").read_text())
    assert doc["frames_total"] == 20 and [p["id"] for p in doc["people"]] == [8, 3, "left"]
    for p, o in zip(doc["people"], outs):
        assert (p["first_frame"], p["last_frame"], p["n_frames"]) == (2, 1 + len(o["frames"]), len(o["frames"]))
        assert p["mean_box_area"] == float((o["bboxes"][:, 2] * o["bboxes"][:, 3]).mean())
        for title in ("REBA", "RULA"):
            final, _, _, (level, name) = o[title.lower()]
            want = [None if np.isnan(v) else float(v) for v in final]
            assert [p[title][k] for k in ("avg", "top50", "top10", "max", "mode")] == want
            assert p[title]["action_level"] == level and p[title]["action"] == name
    assert doc["people"][2]["REBA"]["top10"] is None                      # 5 frames: no top 10 %


def test_persons_all_with_debug_writes_every_persons_csvs_from_its_own_log_slice(tmp_path, monkeypatch):
    smpl = types.SimpleNamespace(joints_name_upper=[f"J{i}" for i in range(22)] + ["L_HIP", "NECK"])
    knobs = dict(debugging=True, debug_joints=["L_Hip", "Neck"], smpl_model=smpl)
    pred = _bare_predictor(persons="all", **knobs)
    outs = [_canned(pred.reba, pred.rula, n, s) for n, s in ((12, 1), (9, 2), (5, 3))]
    slices = [{"reba": [REBA._angle_log(p) for p in o["result"]], "rula": [RULA._angle_log(p) for p in o["result"]]} for o in outs]
    people = {"people": outs, "ids": [8, 3, "left"], "frames_total": 20, "pose_logs": slices}
    # the scorers' own logs hold every person's rows, the target's first: what one pass over everybody leaves behind
    pred.reba.log = [row for s in slices for row in s["reba"]]
    pred.rula.log = [row for s in slices for row in s["rula"]]
    monkeypatch.setattr(base.Predictor, "score_people", lambda self, *a, **k: people)
    monkeypatch.setattr(base.Predictor, "score_frames", lambda self, *a, **k: pytest.fail("the model must run once"))
    frames = np.zeros((20, 8, 8, 3), np.uint8)
    pred(None, None, str(tmp_path / "all"), frames=frames, tracking_results={1: None})
    per_person = ["REBA_score.png", "RULA_score.png", "reba_result.txt", "rula_result.txt"]
    csvs = ["REBA_eval_pose_log.csv", "REBA_score_log.csv", "RULA_eval_pose_log.csv", "RULA_score_log.csv", "pose_log.csv"]
    assert _files(tmp_path / "all") == sorted(per_person + ["people.json"] + [f"debug/{f}" for f in csvs] +
                                              [f"person_{i}/{f}" for i in (8, 3, "left") for f in per_person + csvs])
    # the target's folder holds what a 'target' run on the same canned target writes under debug/
    one = _bare_predictor(**knobs)
    one.reba.log, one.rula.log = list(slices[0]["reba"]), list(slices[0]["rula"])
    monkeypatch.setattr(base.Predictor, "score_frames", lambda self, *a, **k: dict(outs[0]))
    one(None, None, str(tmp_path / "one"), frames=frames, tracking_results={1: None})
    assert _files(tmp_path / "one") == sorted(per_person + [f"debug/{f}" for f in csvs])
    for f in ("REBA_score_log.csv", "REBA_eval_pose_log.csv", "pose_log.csv"):
        assert (tmp_path / "all" / "person_8" / f).read_bytes() == (tmp_path / "one" / "debug" / f).read_bytes(), f
    # another person's pose-evaluation log is its own slice: frames 2 .. 10 of 20, one row each, its own angles
    import csv
    rows = list(csv.reader(open(tmp_path / "all" / "person_3" / "REBA_eval_pose_log.csv", newline="")))
    names = list(slices[1]["reba"][0])
    assert rows[0] == ["Frame", ""] + names and len(rows) == 1 + 20
    for i in range(20):
        want = [str(i)] + ([""] + [str(slices[1]["reba"][i - 2][n]) for n in names] if 2 <= i < 11 else [])
        assert rows[1 + i] == want, i
    assert slices[1]["reba"][0] != slices[0]["reba"][0]
    assert rows[3][2:] != [str(slices[0]["reba"][0][n]) for n in names]


def test_persons_knob_values():
    args = types.SimpleNamespace(persons="everyone")
    assert base._knob(args, "persons", "persons", "target") == "everyone"
    assert base._knob(types.SimpleNamespace(), "persons", "persons", "target") == "target"
