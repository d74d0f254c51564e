"""The person detector on the GPU (include/poserisk_hip.h, section j8), every tensor inside guard bands: the letterbox bit for bit,
the network per layer against a float64 reference, the post-processing from head tensors of its own, pr_det_detect end to end,
and the Predictor with cfg.TRACKER.weights on a synthetic weight file.

Tolerances.  Network, per tensor: 4 x the distance of the float32 torch-CPU forward from the float64 one on the same weights and
input -- both are fp32 sums in different orders with the same error bound, so the margin covers the order and nothing more.
Post-processing: 4 x the distance of a float32 numpy evaluation from the float64 one.  End to end: 4 x the distance of the
chained float32 references from the chained float64 ones."""
import ctypes as C
import json
import pickle
import sys
import types

import numpy as np
import pytest
import torch

import det_cases as dc
import det_ref
import guard_band as gb
from conftest import measured
from poserisk_release_amd import detector, sort, synth, y4m

pytestmark = pytest.mark.gpu
_detectors = {}


def _detector(device, size, max_batch=3):
    key = (str(device), size, max_batch)
    if key not in _detectors:
        _detectors[key] = detector.Detector(dc.weights(), img_size=size, device=device, max_batch=max_batch, max_det=detector.MAX_CAND)
    return _detectors[key]


# ---- 1. letterbox -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", dc.LETTERBOX_CASES, ids=[c[0] for c in dc.LETTERBOX_CASES])
def test_letterbox_is_bit_exact(gpu_device, case):
    _, H, W, S_h, S_w, bgr, B = case
    det = _detector(gpu_device, (S_h, S_w))
    frames = dc.frames(5, B, H, W)
    want = det_ref.letterbox(frames, S_h, S_w, bgr)
    outs = gb.run_guarded(lambda i, o: det.letterbox(i["frames"], bgr, out=o["x"]), {"frames": torch.from_numpy(frames)},
                          {"x": ((B, S_h, S_w, 4), torch.float32)}, device=gpu_device)
    got = outs["x"].cpu().numpy()
    bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
    assert bad.size == 0, f"{len(bad)} values differ, first (frame, row, col, channel) {bad[0].tolist()}: {got[tuple(bad[0])]!r} for {want[tuple(bad[0])]!r}"


# ---- 2. network ---------------------------------------------------------------------------------------------------------------
_net_refs = {}


def _net_ref(size):
    """(x f32[3,S_h,S_w,4], float64 outputs, float32 outputs) for three letterboxed noise frames: made once a size."""
    if size not in _net_refs:
        x = det_ref.letterbox(dc.frames(7, 3, size[0] - 9, size[1] + 11), size[0], size[1])
        _net_refs[size] = (x, det_ref.forward(dc.weights(), x, torch.float64), det_ref.forward(dc.weights(), x, torch.float32))
    return _net_refs[size]


@pytest.mark.parametrize("B", dc.NETWORK_BATCHES)
@pytest.mark.parametrize("size", dc.NETWORK_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_network_heads_and_layers_against_float64(gpu_device, size, B):
    det = _detector(gpu_device, size)
    x, ref64, ref32 = _net_ref(size)
    shapes = {f"layer{l}": ((B,) + det.layer_shape(l), torch.float32) for l in dc.NETWORK_LAYERS}
    for l in dc.NETWORK_LAYERS:
        assert shapes[f"layer{l}"][0] == (B,) + ref64[l].shape[1:], l
    shapes.update({f"head{i}": ((B, gh, gw, 255), torch.float32) for i, (gh, gw) in enumerate(det.grids)})

    def run(i, o):
        det.network(i["x"], out=[o["head0"], o["head1"], o["head2"]])
        for l in dc.NETWORK_LAYERS:
            det.network_until(i["x"], l, out=o[f"layer{l}"])

    outs = gb.run_guarded(run, {"x": torch.from_numpy(x[:B])}, shapes, device=gpu_device)
    failures = []
    for name, l in [(f"head{i}", h) for i, h in enumerate(detector.HEAD_LAYERS)] + [(f"layer{l}", l) for l in dc.NETWORK_LAYERS]:
        got = outs[name].cpu().numpy().astype(np.float64)
        yard = float(np.abs(ref32[l][:B].astype(np.float64) - ref64[l][:B]).max())
        err = float(np.abs(got - ref64[l][:B]).max())
        measured(f"det {size[0]}x{size[1]} B{B} {name} fp32-cpu", yard)
        measured(f"det {size[0]}x{size[1]} B{B} {name} gpu", err, 4 * yard)
        if not err <= 4 * yard:
            failures.append(f"{name}: {err:.3e} > 4 x {yard:.3e}")
    # the heads through pr_det_network are the bits of the yolo layers through pr_det_network_until
    for i, h in enumerate(detector.HEAD_LAYERS):
        assert torch.equal(outs[f"head{i}"], outs[f"layer{h}"]), h
    assert not failures, failures


def test_network_refuses_by_name(gpu_device):
    det = _detector(gpu_device, (32, 64))
    x = torch.zeros((4, 32, 64, 4), device=gpu_device)
    with pytest.raises(detector._lib.PoseRiskHipError, match="max_batch = 3"):
        det.network(x)
    with pytest.raises(detector._lib.PoseRiskHipError, match="layer = 107"):
        det.network_until(x[:1], 107, out=torch.zeros((1, 1, 2, 255), device=gpu_device))
    with pytest.raises(detector._lib.PoseRiskHipError, match="multiples of 32"):
        detector.Detector(dc.weights(), img_size=(48, 64), device=gpu_device, max_batch=1)
    with pytest.raises(detector._lib.PoseRiskHipError, match="n_floats"):
        detector.Detector(dc.weights()[:-1], img_size=(32, 64), device=gpu_device, max_batch=1)


# ---- 3. post-processing from its own input --------------------------------------------------------------------------------------
def _assert_margins(cells, order, ious, what):
    """The float64 reference is not too close to call anywhere: the issue's three margins."""
    person = cells["person"]
    assert not np.any(np.abs(cells["obj"][person] - dc.CONF) < dc.OBJ_MARGIN), f"{what}: an objectness within {dc.OBJ_MARGIN} of conf_thres"
    s = np.sort(cells["score"][order])
    assert s.size < 2 or np.diff(s).min() > dc.SCORE_MARGIN, f"{what}: two scores within {dc.SCORE_MARGIN}"
    off = ious[~np.eye(len(order), dtype=bool)]
    assert not np.any(np.abs(off - dc.NMS) < dc.IOU_MARGIN), f"{what}: a pair's IoU within {dc.IOU_MARGIN} of nms_thres"


def _post_reference(heads):
    c64, c32 = det_ref.decode(heads, np.float64), det_ref.decode(heads, np.float32)
    out = []
    for b, (a, f) in enumerate(zip(c64, c32)):
        order, kept, overflow, ious = det_ref.select(a, dc.CONF, dc.NMS)
        _assert_margins(a, order, ious, f"frame {b}")
        out.append({"kept": kept, "overflow": overflow, "n_cand": int(((a["obj"] >= dc.CONF) & a["person"]).sum()),
                    "box": a["box"][kept], "score": a["score"][kept],
                    "box_tol": 4 * float(np.abs(f["box"][kept].astype(np.float64) - a["box"][kept]).max()) if kept.size else 0.0,
                    "score_tol": 4 * float(np.abs(f["score"][kept].astype(np.float64) - a["score"][kept]).max()) if kept.size else 0.0})
    return out


def _compare_post(got, ref, b, what):
    boxes, scores, count, status = got
    n = int(count[b])
    assert n == ref["kept"].size, f"{what} frame {b}: {n} boxes, the reference keeps {ref['kept'].size}"
    if n:
        eb = float(np.abs(boxes[b, :n].astype(np.float64) - ref["box"]).max())
        es = float(np.abs(scores[b, :n].astype(np.float64) - ref["score"]).max())
        measured(f"det {what} frame {b} boxes", eb, ref["box_tol"], "px")
        measured(f"det {what} frame {b} scores", es, ref["score_tol"])
        assert eb <= ref["box_tol"] and es <= ref["score_tol"], (what, b, eb, ref["box_tol"], es, ref["score_tol"])
    assert not boxes[b, n:].any() and not scores[b, n:].any(), f"{what} frame {b}: rows beyond count are not zero"


@pytest.mark.parametrize("B", (1, 3))
def test_postprocess_from_crafted_heads(gpu_device, B):
    det = _detector(gpu_device, dc.POST_SIZE)
    heads = [h[:B] for h in dc.crafted_heads(*dc.POST_SIZE)]
    ref = _post_reference(heads)
    assert ref[0]["n_cand"] > 60 and ref[0]["kept"].size < ref[0]["n_cand"]          # NMS has work in frame 0
    M = detector.MAX_CAND
    outs = gb.run_guarded(lambda i, o: det.postprocess([i["h0"], i["h1"], i["h2"]], dc.CONF, dc.NMS, M, out=o),
                          {f"h{k}": torch.from_numpy(h) for k, h in enumerate(heads)},
                          {"boxes": ((B, M, 4), torch.float32), "scores": ((B, M), torch.float32), "count": ((B,), torch.int32),
                           "status": ((B,), torch.int32)}, device=gpu_device)
    got = [outs[k].cpu().numpy() for k in ("boxes", "scores", "count", "status")]
    for b in range(B):
        _compare_post(got, ref[b], b, f"post B{B}")
        assert int(got[3][b]) == (detector.STATUS_CAND_OVERFLOW if ref[b]["overflow"] else 0), b
    if B == 3:
        assert ref[1]["n_cand"] == 0 and got[2][1] == 0                               # a frame with no candidate
        assert ref[2]["n_cand"] > M and ref[2]["overflow"] and ref[2]["kept"].size > 1000       # the cut is reported, never silent


def test_postprocess_reports_more_boxes_than_max_det(gpu_device):
    det = _detector(gpu_device, dc.POST_SIZE)
    heads = [torch.from_numpy(h[:1]).to(gpu_device) for h in dc.crafted_heads(*dc.POST_SIZE)]
    ref = _post_reference([h.cpu().numpy() for h in heads])[0]
    boxes, scores, count, status = (t.cpu().numpy() for t in det.postprocess(heads, dc.CONF, dc.NMS, 5))
    assert count[0] == 5 and status[0] == detector.STATUS_DET_OVERFLOW
    assert np.abs(boxes[0].astype(np.float64) - ref["box"][:5]).max() <= ref["box_tol"]
    with pytest.raises(detector._lib.PoseRiskHipError, match="max_det = 0"):
        det.postprocess(heads, dc.CONF, dc.NMS, 0)
    with pytest.raises(detector._lib.PoseRiskHipError, match="conf_thres"):
        det.postprocess(heads, 1.5, dc.NMS, 5)


# ---- 3b. post-processing ON its contract's edges: ties, thresholds met exactly, empty boxes, the cut, non-finite values -------------
# No margins here (_assert_margins is for the tolerance tests above): the crafted cells have tx = ty = tw = th = 0, so their boxes
# and IoUs are exact in fp32 and the reference is the contract to the letter, det_ref.decode(heads, float64, float32).
def _run_post(det, heads, conf, nms, max_det, device):
    B = heads[0].shape[0]
    outs = gb.run_guarded(lambda i, o: det.postprocess([i["h0"], i["h1"], i["h2"]], conf, nms, max_det, out=o),
                          {f"h{k}": torch.from_numpy(np.ascontiguousarray(h)) for k, h in enumerate(heads)},
                          {"boxes": ((B, max_det, 4), torch.float32), "scores": ((B, max_det), torch.float32), "count": ((B,), torch.int32),
                           "status": ((B,), torch.int32)}, device=device)
    return [outs[k].cpu().numpy() for k in ("boxes", "scores", "count", "status")]


def _edge_reference(heads, conf, nms):
    """Per frame: the contract's kept flat indices in order, its fp32 boxes (exact where the box logits are 0), the float64 scores and
    the tolerance for them (the score_tol rule: 4 x |float32 evaluation - float64|), and the status word without DET_OVERFLOW."""
    c64, c32, cc = det_ref.decode(heads, np.float64), det_ref.decode(heads, np.float32), det_ref.decode(heads, np.float64, np.float32)
    out = []
    for a, f, c in zip(c64, c32, cc):
        order, kept, overflow, _ = det_ref.select(c, conf, nms)
        status = (detector.STATUS_CAND_OVERFLOW if overflow else 0) | (detector.STATUS_NONFINITE if det_ref.candidates(c, conf)[1] else 0)
        out.append({"order": order, "kept": kept, "status": status, "box32": c["box"][kept], "box": a["box"][kept], "score": a["score"][kept],
                    "box_tol": 4 * float(np.abs(f["box"][kept].astype(np.float64) - a["box"][kept]).max()) if kept.size else 0.0,
                    "score_tol": 4 * float(np.abs(f["score"][kept].astype(np.float64) - a["score"][kept]).max()) if kept.size else 0.0})
    return out


def _assert_edge(got, ref, b, what, exact_boxes=True):
    boxes, scores, count, status = got
    n = int(count[b])
    assert n == ref["kept"].size, f"{what} frame {b}: {n} boxes, the contract keeps {ref['kept'].size} (cells {ref['kept'].tolist()[:8]})"
    assert int(status[b]) == ref["status"], (what, b, int(status[b]), ref["status"])
    if n:
        if exact_boxes:
            assert np.array_equal(boxes[b, :n], ref["box32"]), f"{what} frame {b}: boxes\n{boxes[b, :n]}\nfor\n{ref['box32']}"
        else:
            eb = float(np.abs(boxes[b, :n].astype(np.float64) - ref["box"]).max())
            print(f"[edge] {what} frame {b} boxes: {eb:.3e} px (tolerance {ref['box_tol']:g})")
            assert eb <= ref["box_tol"], (what, b, eb, ref["box_tol"])
        es = float(np.abs(scores[b, :n].astype(np.float64) - ref["score"]).max())
        print(f"[edge] {what} frame {b} scores: {es:.3e} (tolerance {ref['score_tol']:g})")
        assert es <= ref["score_tol"], (what, b, es, ref["score_tol"])
    assert not boxes[b, n:].any() and not scores[b, n:].any(), f"{what} frame {b}: rows beyond count are not zero"


def _edge_case(gpu_device, cells, conf, nms, want_kept, what, max_det=16):
    """Run the named cells; the kept cells, in order, must be `want_kept` by the contract reference AND on the GPU."""
    det = _detector(gpu_device, dc.POST_SIZE)
    heads = dc.edge_heads(cells)
    ref = _edge_reference(heads, conf, nms)[0]
    assert ref["kept"].tolist() == [dc.flat_index(c) for c in want_kept], (what, ref["kept"].tolist())
    got = _run_post(det, heads, conf, nms, max_det, gpu_device)
    _assert_edge(got, ref, 0, what)
    return got, ref


def test_nms_drops_only_above_the_threshold_never_at_it(gpu_device):
    cells = {dc.EDGE_A: {"tc0": 0.0}, dc.EDGE_B: {"tc0": -1.0}}
    at = float(dc.EDGE_IOU_1)
    below = float(np.nextafter(dc.EDGE_IOU_1, np.float32(0)))
    assert np.float32(at) == dc.EDGE_IOU_1 and np.float32(below) < dc.EDGE_IOU_1
    _edge_case(gpu_device, cells, 0.1, at, [dc.EDGE_A, dc.EDGE_B], "IoU == nms_thres")
    _edge_case(gpu_device, cells, 0.1, below, [dc.EDGE_A], "IoU one ulp above nms_thres")


def test_objectness_equal_to_the_threshold_is_a_candidate(gpu_device):
    cells = {dc.EDGE_B: {}}
    above = float(np.nextafter(np.float32(0.5), np.float32(1)))
    got, _ = _edge_case(gpu_device, cells, 0.5, 0.4, [dc.EDGE_B], "obj == conf_thres")
    assert got[2][0] == 1
    got, _ = _edge_case(gpu_device, cells, above, 0.4, [], "obj one ulp below conf_thres")
    assert got[2][0] == 0


TIE_PAIRS = {"one column apart": (dc.EDGE_A, dc.EDGE_B), "head 32 and head 16": (dc.EDGE_B, dc.EDGE_B16), "two anchors of a cell": dc.EDGE_ANCHOR_PAIR}


@pytest.mark.parametrize("pair", TIE_PAIRS, ids=[k.replace(" ", "-") for k in TIE_PAIRS])
def test_equal_scores_are_ordered_by_the_flat_index(gpu_device, pair):
    first, second = TIE_PAIRS[pair]
    assert dc.flat_index(first) < dc.flat_index(second)
    cells = {second: {}, first: {}}
    got, ref = _edge_case(gpu_device, cells, 0.1, 0.4, [first], pair)
    assert got[1][0, 0] == np.float32(0.25)
    got, ref = _edge_case(gpu_device, cells, 0.1, 1.0, [first, second], pair + ", nms_thres = 1")
    assert got[1][0, 0] == got[1][0, 1] == np.float32(0.25)


def test_only_a_kept_box_suppresses(gpu_device):
    cells = {dc.EDGE_A: {"tc0": 0.0}, dc.EDGE_B: {"tc0": -1.0}, dc.EDGE_C: {"tc0": -2.0}}
    _edge_case(gpu_device, cells, 0.1, 0.4, [dc.EDGE_A, dc.EDGE_C], "A > B > C")


@pytest.mark.parametrize("nms", (0.4, 0.0))
def test_empty_boxes_overlap_nothing(gpu_device, nms):
    hd, _, cy, cx = dc.EDGE_B
    e0, e1, big = (hd, 0, cy, cx), (hd, 1, cy, cx), (hd, 2, cy, cx)
    empty = {"box": (0, 0, -200, -200), "tc0": -1.0}
    got, ref = _edge_case(gpu_device, {e0: empty, e1: empty}, 0.1, nms, [e0, e1], "two empty boxes: 0 / 0")
    assert np.array_equal(got[0][0, :2], np.array([[48, 48, 48, 48]] * 2, np.float32))
    # inside the 373 x 326 box of the same cell, which is kept first: IoU 0 / area = 0
    got, ref = _edge_case(gpu_device, {e0: empty, e1: empty, big: {}}, 0.1, nms, [big, e0, e1], "empty boxes inside a kept one")
    assert np.array_equal(got[0][0, 0], np.array([48 - 186.5, 48 - 163, 48 + 186.5, 48 + 163], np.float32))


@pytest.mark.parametrize("n,tie", ((detector.MAX_CAND, False), (detector.MAX_CAND + 1, False), (detector.MAX_CAND + 1, True)),
                         ids=("exactly-MAX_CAND", "one-more", "one-more-tied-at-the-cut"))
def test_the_cut_at_max_cand(gpu_device, n, tie):
    """nms_thres = 1 keeps every participant, so the output IS the list of those that took part, in order."""
    M = detector.MAX_CAND
    det = _detector(gpu_device, dc.POST_SIZE)
    heads, pick = dc.cut_heads(n, tie)
    ref = _edge_reference(heads, 0.1, 1.0)[0]
    flats = np.array([dc.flat_index(c) for c in pick])
    score = det_ref.decode(heads)[0]["score"]
    by_rank = flats[np.lexsort((flats, -score[flats]))]
    assert ref["kept"].size == M and np.array_equal(ref["kept"], by_rank[:M])
    assert ref["status"] == (detector.STATUS_CAND_OVERFLOW if n > M else 0)
    if tie:      # ranks M - 1 and M hold one score: the lower flat index takes part
        assert score[by_rank[M - 1]] == score[by_rank[M]] and by_rank[M - 1] < by_rank[M]
    got = _run_post(det, heads, 0.1, 1.0, M, gpu_device)
    _assert_edge(got, ref, 0, f"cut {n} tie {tie}", exact_boxes=False)


def test_frames_are_independent_and_runs_reproduce(gpu_device):
    det = _detector(gpu_device, dc.POST_SIZE)
    heads = dc.crafted_heads(*dc.POST_SIZE)
    M = detector.MAX_CAND
    whole = _run_post(det, heads, dc.CONF, dc.NMS, M, gpu_device)
    again = _run_post(det, heads, dc.CONF, dc.NMS, M, gpu_device)
    for name, a, b in zip(("boxes", "scores", "count", "status"), whole, again):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), f"{name}: a second run of the same call gives other bits"
    for b in range(3):
        alone = _run_post(det, [h[b:b + 1] for h in heads], dc.CONF, dc.NMS, M, gpu_device)
        for name, a, w in zip(("boxes", "scores", "count", "status"), alone, whole):
            assert np.array_equal(a[0].view(np.uint32), w[b].view(np.uint32)), f"frame {b} {name}: alone is not what it is in a batch of 3"


def _poison(kind):
    """Three copies of crafted_heads' frame 0, frame 1 poisoned in its best kept cell -> (clean heads, poisoned heads)."""
    clean = [np.repeat(h[:1], 3, axis=0) for h in dc.crafted_heads(*dc.POST_SIZE)]
    cells = det_ref.decode([h[:1] for h in clean], np.float64, np.float32)[0]
    flat = int(det_ref.select(cells, dc.CONF, dc.NMS)[1][0])
    hd, a, cy, cx = dc.all_cells()[flat]
    assert dc.flat_index((hd, a, cy, cx)) == flat
    bad = [h.copy() for h in clean]
    channel, value = {"to-nan": (4, np.nan), "tc0-nan": (5, np.nan), "tw-inf": (2, np.inf), "tw-89": (2, 89.0), "tx-nan": (0, np.nan),
                      "class7-nan": (5 + 7, np.nan)}[kind]
    bad[hd][1, cy, cx, a * 85 + channel] = value
    return clean, bad, flat


@pytest.mark.parametrize("kind", ("to-nan", "tc0-nan", "tw-inf", "tw-89", "tx-nan", "class7-nan"))
def test_a_non_finite_head_value_takes_its_cell_out_and_is_reported(gpu_device, kind):
    det = _detector(gpu_device, dc.POST_SIZE)
    clean, bad, flat = _poison(kind)
    M = detector.MAX_CAND
    ref_clean, ref = _edge_reference(clean, dc.CONF, dc.NMS), _edge_reference(bad, dc.CONF, dc.NMS)
    harmless = kind == "class7-nan"
    assert (flat in ref[1]["kept"]) == harmless and ref[1]["status"] == (0 if harmless else detector.STATUS_NONFINITE)
    assert flat in ref_clean[1]["order"] and (flat in ref[1]["order"]) == harmless
    assert np.array_equal(ref[0]["kept"], ref_clean[0]["kept"]) and ref[0]["status"] == ref[2]["status"] == 0
    if kind == "tw-89":      # finite in float64, infinite in fp32 only
        assert np.isfinite(det_ref.decode([h[1:2] for h in bad])[0]["box"][flat]).all()
    want = _run_post(det, clean, dc.CONF, dc.NMS, M, gpu_device)
    got = _run_post(det, bad, dc.CONF, dc.NMS, M, gpu_device)
    again = _run_post(det, bad, dc.CONF, dc.NMS, M, gpu_device)
    for name, g, w, r in zip(("boxes", "scores", "count", "status"), got, want, again):
        assert np.array_equal(g.view(np.uint32), r.view(np.uint32)), f"{name}: a second run gives other bits"
        for b in (0, 2):
            assert np.array_equal(g[b].view(np.uint32), w[b].view(np.uint32)), f"frame {b} {name}: changed by a value in frame 1"
    assert not want[3].any() and got[3][0] == 0 and got[3][2] == 0
    _assert_edge(got, ref[1], 1, kind, exact_boxes=False)
    if harmless:
        assert np.array_equal(got[0][1].view(np.uint32), want[0][1].view(np.uint32)) and got[3][1] == 0


# ---- 3c. the map back to the frame, alone ---------------------------------------------------------------------------------------
def test_unmap_geometries_cover_both_bars_and_both_scale_directions():
    geo = [(H, W) + detector.letterbox_geometry(H, W, S_h, S_w) for H, W, S_h, S_w in dc.UNMAP_GEOMETRIES]      # H, W, h', w', ox, oy
    assert {c[1:5] for c in dc.LETTERBOX_CASES} <= set(dc.UNMAP_GEOMETRIES)
    assert {(1080, 1920, 416, 416), (1920, 1080, 416, 416), (1, 1, 32, 32)} <= set(dc.UNMAP_GEOMETRIES)
    assert any(max(g[:2]) == 4096 for g in dc.UNMAP_GEOMETRIES)                       # PR_RESIZE_MAX_SIDE
    assert any(ox > 0 and oy == 0 for *_, ox, oy in geo) and any(oy > 0 and ox == 0 for *_, ox, oy in geo)
    sx = [np.float32(W) / np.float32(w2) for H, W, h2, w2, ox, oy in geo]
    sy = [np.float32(H) / np.float32(h2) for H, W, h2, w2, ox, oy in geo]
    assert max(sx) > 1 and min(sx) < 1 and max(sy) > 1 and min(sy) < 1 and any(a != b for a, b in zip(sx, sy))


@pytest.mark.parametrize("geometry", dc.UNMAP_GEOMETRIES, ids=lambda g: "x".join(str(v) for v in g))
def test_unmap_alone_is_bit_exact(gpu_device, geometry):
    """A subtraction, a multiplication by one rounded fp32 quotient and two clamps, each rounded, none fusable: equality."""
    H, W, S_h, S_w = geometry
    h2, w2, ox, oy = detector.letterbox_geometry(H, W, S_h, S_w)
    boxes, kinds = dc.unmap_boxes(h2, w2, ox, oy, S_h, S_w)
    count = np.array(dc.UNMAP_COUNTS, np.int32)
    want = boxes.copy()
    for b, n in enumerate(count):
        want[b, :n] = det_ref.unmap(boxes[b, :n], H, W, S_h, S_w, np.float32)
    assert want.dtype == np.float32
    # what the reference itself says of the crafted rows: a box inside a padding bar comes out empty, on the frame's edge
    f0 = want[0]
    assert (f0[kinds["bar_x"], 0] == f0[kinds["bar_x"], 2]).all() and f0[kinds["bar_x"], 0].tolist() == [0.0, float(W)]
    assert (f0[kinds["bar_y"], 1] == f0[kinds["bar_y"], 3]).all() and f0[kinds["bar_y"], 1].tolist() == [0.0, float(H)]
    assert f0[kinds["corners"][0]].tolist() == [0.0, 0.0, float(W), float(H)]
    assert (f0[kinds["inside"], 2] > f0[kinds["inside"], 0]).all() and (f0[kinds["inside"], 3] > f0[kinds["inside"], 1]).all()
    assert (f0[:, 0::2] >= 0).all() and (f0[:, 0::2] <= W).all() and (f0[:, 1::2] >= 0).all() and (f0[:, 1::2] <= H).all()
    ins = {"boxes": torch.from_numpy(boxes), "count": torch.from_numpy(count)}
    got = {}

    def run(i, o):
        detector.unmap(i["boxes"], i["count"], (H, W), (S_h, S_w))
        got["boxes"] = i["boxes"].cpu().numpy()

    gb.run_guarded(run, ins, {}, device=gpu_device, mutated=("boxes",))
    g = got["boxes"]
    for b, n in enumerate(count):
        assert np.array_equal(g[b, n:].view(np.uint32), boxes[b, n:].view(np.uint32)), f"frame {b}: a row at or beyond count {n} was touched"
    bad = np.argwhere(g.view(np.uint32) != want.view(np.uint32))
    assert bad.size == 0, (f"{len(bad)} values differ, first (frame, row, corner) {bad[0].tolist()}: {g[tuple(bad[0])]!r} for "
                           f"{want[tuple(bad[0])]!r} from {boxes[tuple(bad[0])]!r}")


def test_unmap_refuses_by_name(gpu_device):
    boxes = torch.zeros((2, 4, 4), device=gpu_device)
    count = torch.zeros((2,), dtype=torch.int32, device=gpu_device)
    lib = detector._lib.load()
    for args, name in (((None, count.data_ptr(), 2, 4, 54, 96, 64, 96), "null boxes_dev"), ((boxes.data_ptr(), None, 2, 4, 54, 96, 64, 96), "null count_dev"),
                       ((boxes.data_ptr(), count.data_ptr(), -1, 4, 54, 96, 64, 96), "B = -1"),
                       ((boxes.data_ptr(), count.data_ptr(), 2, 0, 54, 96, 64, 96), "max_det = 0"),
                       ((boxes.data_ptr(), count.data_ptr(), 2, 4, 0, 96, 64, 96), "frames of 96 x 0"),
                       ((boxes.data_ptr(), count.data_ptr(), 2, 4, 54, 4097, 64, 96), "frames of 4097 x 54"),
                       ((boxes.data_ptr(), count.data_ptr(), 2, 4, 54, 96, 48, 96), "multiples of 32")):
        with pytest.raises(detector._lib.PoseRiskHipError, match="pr_det_unmap: .*" + name):
            detector._lib.check(lib.pr_det_unmap(*args, None), "pr_det_unmap")
    detector._lib.check(lib.pr_det_unmap(boxes.data_ptr(), count.data_ptr(), 0, 4, 54, 96, 64, 96, None), "pr_det_unmap")      # B = 0: PR_OK
    with pytest.raises(ValueError, match="boxes must be"):
        detector.unmap(boxes[:, :, :3].contiguous(), count, (54, 96), (64, 96))


# ---- 4. pr_det_detect end to end ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", dc.DETECT_CASES, ids=lambda c: f"{c[0]}x{c[1]}" + ("-bgr" if c[2] else ""))
def test_detect_end_to_end_against_the_chained_references(gpu_device, case):
    S_h, S_w = dc.DETECT_SIZE
    H, W, bgr = case
    B = 3
    det = _detector(gpu_device, dc.DETECT_SIZE)
    frames = dc.frames(dc.DETECT_SEED, B, H, W)
    x = det_ref.letterbox(frames, S_h, S_w, bgr)
    h2, w2, ox, oy = detector.letterbox_geometry(H, W, S_h, S_w)
    in_a_bar = 0
    chains = {}
    for name, tdt, ndt in (("f64", torch.float64, np.float64), ("f32", torch.float32, np.float32)):
        o = det_ref.forward(dc.weights(), x, tdt)
        chains[name] = det_ref.decode([o[l].astype(np.float32) for l in detector.HEAD_LAYERS], ndt)
    M = 256
    outs = gb.run_guarded(lambda i, o: det.detect_raw(i["frames"], bgr, dc.CONF, dc.NMS, M, out=o), {"frames": torch.from_numpy(frames)},
                          {"boxes": ((B, M, 4), torch.float32), "scores": ((B, M), torch.float32), "count": ((B,), torch.int32),
                           "status": ((B,), torch.int32)}, device=gpu_device)
    boxes, scores, count, status = (outs[k].cpu().numpy() for k in ("boxes", "scores", "count", "status"))
    total = left_out = compared = 0
    for b in range(B):
        a, f = chains["f64"][b], chains["f32"][b]
        order, kept, overflow, ious = det_ref.select(a, dc.CONF, dc.NMS)
        total += order.size
        try:
            _assert_margins(a, order, ious, f"frame {b}")
        except AssertionError:
            left_out += order.size      # a frame with a candidate too close to call is left out whole
            continue
        _, kept32, _, _ = det_ref.select(f, dc.CONF, dc.NMS)
        assert np.array_equal(kept, kept32), f"frame {b}: the float32 chain keeps another set"
        lb = a["box"][kept]
        in_a_bar += int(((lb[:, 2] <= ox) | (lb[:, 0] >= ox + w2) | (lb[:, 3] <= oy) | (lb[:, 1] >= oy + h2)).sum())
        want = det_ref.unmap(a["box"][kept], H, W, S_h, S_w, np.float64)
        yard = det_ref.unmap(f["box"][kept], H, W, S_h, S_w, np.float32).astype(np.float64)
        assert int(count[b]) == kept.size and status[b] == 0, (b, int(count[b]), kept.size)
        if kept.size:
            tb, ts = 4 * float(np.abs(yard - want).max()), 4 * float(np.abs(f["score"][kept].astype(np.float64) - a["score"][kept]).max())
            eb = float(np.abs(boxes[b, :kept.size].astype(np.float64) - want).max())
            es = float(np.abs(scores[b, :kept.size].astype(np.float64) - a["score"][kept]).max())
            measured(f"det detect {H}x{W}{' bgr' if bgr else ''} frame {b} boxes", eb, tb, "px")
            measured(f"det detect {H}x{W}{' bgr' if bgr else ''} frame {b} scores", es, ts)
            assert eb <= tb and es <= ts, (b, eb, tb, es, ts)
            compared += kept.size
    assert total >= 20 and compared > 0, (total, compared)
    assert left_out <= 0.02 * total, f"{left_out} of {total} reference candidates left out"
    if (H, W) == (97, 41):      # the clip has work: kept boxes wholly inside a padding bar, which come out empty on the frame's edge
        assert in_a_bar >= 1, "no reference box lies wholly inside a padding bar"


# ---- 5. the Predictor with the built-in tracker ---------------------------------------------------------------------------------
@pytest.fixture(scope="session")
def weight_file(tmp_path_factory):
    path = tmp_path_factory.mktemp("yolo") / "synthetic.weights"
    detector.save_darknet(path, dc.weights())
    return str(path)


def test_predictor_tracks_with_the_built_in_detector(gpu_device, tmp_path, monkeypatch, weight_file):
    from poserisk_release_amd import dropin
    dropin.install()
    from core import base
    from core.config import cfg
    from models import hmr
    from smpl import SMPL
    monkeypatch.setitem(sys.modules, "cv2", None)
    monkeypatch.setitem(sys.modules, "multi_person_tracker", None)
    W, H, n = 320, 180, 8
    rng = np.random.default_rng(1)
    still = rng.integers(0, 256, (H, W), dtype=np.uint8)
    Y = np.clip(still[None].astype(np.int16) + rng.integers(-1, 2, (n, H, W)), 0, 255).astype(np.uint8)
    U = np.broadcast_to(rng.integers(96, 160, (1, H // 2, W // 2), dtype=np.uint8), (n, H // 2, W // 2)).copy()
    V = np.broadcast_to(rng.integers(96, 160, (1, H // 2, W // 2), dtype=np.uint8), (n, H // 2, W // 2)).copy()
    clip = tmp_path / "clip.y4m"
    y4m.write(clip, Y, U, V, fps=(24, 1), chroma="420mpeg2")
    (tmp_path / "info.json").write_text(json.dumps(synth.EXAMPLE_INFO))
    model = hmr()
    model.load_state_dict(synth.hmr_state_dict(seed=1), strict=False)
    smpl = SMPL(models={"neutral": synth.smpl_model(V=6890, seed=2)}, device=gpu_device)
    args = types.SimpleNamespace(gpu="0", type="REBA,RULA", debug=False, debug_joints="", debug_frame=-1)
    pred = base.Predictor(args, spin_model=model, smpl_model=smpl, batch_size=4)
    # the knob unset: today's error, word for word
    assert cfg.TRACKER.weights == ""
    with pytest.raises(RuntimeError, match=r"8 frames of 320 x 180 were decoded, but there is no tracking for them: .*clip\.tracking\.pkl.* does not "
                                           r"exist, no tracking_results were given and multi_person_tracker is not importable here"):
        pred(str(clip), str(tmp_path / "info.json"), str(tmp_path / "out0"))
    monkeypatch.setitem(cfg.TRACKER, "weights", weight_file)
    monkeypatch.setitem(cfg.TRACKER, "img_size", (64, 96))
    monkeypatch.setitem(cfg.TRACKER, "batch", 3)
    out = pred(str(clip), str(tmp_path / "info.json"), str(tmp_path / "out"))
    decoded = y4m.decode(str(clip), gpu_device)
    dets = detector.Detector(weight_file, img_size=(64, 96), device=gpu_device, max_batch=3).detect(decoded, conf_thres=0.1, nms_thres=0.4)
    tracking = sort.track_frames(dets)
    assert tracking and max(len(t["frames"]) for t in tracking.values()) >= 3
    again = pred.track_frames(decoded)
    assert list(again) == list(tracking)
    for k in tracking:
        assert np.array_equal(again[k]["bbox"], tracking[k]["bbox"]) and np.array_equal(again[k]["frames"], tracking[k]["frames"])
    want = pred.score_frames(decoded, tracking, synth.EXAMPLE_INFO)
    assert len(out["frames"]) >= 3
    for k in ("result", "joint_cam", "frames"):
        assert np.array_equal(np.asarray(out[k]), np.asarray(want[k])), k
    for t in ("reba", "rula"):
        np.testing.assert_array_equal(np.asarray(out[t][0], np.float64), np.asarray(want[t][0], np.float64), err_msg=t)
    # a frame folder without tracking.pkl is accepted while the knob is set, and the sidecar the command line writes is the same dict
    folder = tmp_path / "folder"
    folder.mkdir()
    np.save(folder / "frames.npy", decoded.cpu().numpy())
    _, bgr2, fps2, tracking2 = pred.load_front_end(str(folder), str(tmp_path / "out2"))
    assert not bgr2 and fps2 == 30.0 and list(tracking2) == list(tracking)
    assert all(np.array_equal(tracking2[k]["bbox"], tracking[k]["bbox"]) for k in tracking)
    from poserisk_release_amd import frontend
    sidecar, _, n_frames = frontend.track(str(clip), weight_file, out=str(tmp_path / "side.pkl"), device=gpu_device, img_size=(64, 96), batch=3)
    with open(sidecar, "rb") as f:
        loaded = pickle.load(f)
    assert n_frames == n and list(loaded) == list(tracking) and all(np.array_equal(loaded[k]["frames"], tracking[k]["frames"]) for k in tracking)
    # zero tracks: an error that says so, with the threshold used
    monkeypatch.setitem(cfg.TRACKER, "conf_thres", 1.0)
    with pytest.raises(RuntimeError, match=r"found no person track in 8 frames \(0 detections at conf_thres 1"):
        pred.track_frames(decoded)


# ---- 6. the convolution alone, on shapes the network at these sizes does not reach -----------------------------------------------
CONV_CASES = (          # (B, H, W, Cin, Cout, ksize, stride, leaky, residual): odd maps, ragged tiles, more than one block
    (2, 13, 17, 4, 32, 3, 1, True, False),
    (1, 13, 17, 32, 64, 3, 2, True, False),
    (3, 7, 9, 64, 128, 3, 1, True, True),
    (2, 5, 11, 768, 256, 1, 1, True, False),
    (2, 9, 7, 64, 255, 1, 1, False, False),
    (1, 3, 5, 36, 100, 3, 2, False, True),
)


@pytest.mark.parametrize("case", CONV_CASES, ids=lambda c: "x".join(str(int(v)) for v in c))
def test_det_conv_alone_against_float64(gpu_device, case):
    from poserisk_release_amd import ops
    B, H, W, Cin, Cout, k, stride, leaky, with_res = case
    rng = np.random.default_rng(9)
    x = rng.standard_normal((B, H, W, Cin), dtype=np.float32)
    w = rng.standard_normal((Cout, Cin, k, k), dtype=np.float32) * np.float32(np.sqrt(2.0 / (Cin * k * k)))
    b = rng.standard_normal(Cout, dtype=np.float32)
    Ho, Wo = (H + 2 * (k // 2) - k) // stride + 1, (W + 2 * (k // 2) - k) // stride + 1
    res = rng.standard_normal((B, Ho, Wo, Cout), dtype=np.float32) if with_res else None
    cout_pad, kpad = -(-Cout // 64) * 64, -(-(k * k * Cin) // 32) * 32
    packed = np.zeros((cout_pad, kpad), np.float32)
    packed[:Cout, :k * k * Cin] = w.transpose(0, 2, 3, 1).reshape(Cout, -1)
    bias = np.zeros(cout_pad, np.float32)
    bias[:Cout] = b

    def ref(dt):
        y = torch.nn.functional.conv2d(torch.from_numpy(x).to(dt).permute(0, 3, 1, 2), torch.from_numpy(w).to(dt), torch.from_numpy(b).to(dt),
                                       stride=stride, padding=k // 2)
        if leaky:
            y = torch.nn.functional.leaky_relu(y, 0.1)
        y = y.permute(0, 2, 3, 1)
        return (y + torch.from_numpy(res).to(dt) if with_res else y).numpy().astype(np.float64)

    want, yard = ref(torch.float64), ref(torch.float32)
    ins = {"x": torch.from_numpy(x), "packed": torch.from_numpy(np.concatenate([bias, packed.ravel()]))}
    if with_res:
        ins["res"] = torch.from_numpy(res)
    outs = gb.run_guarded(lambda i, o: ops.det_conv_nhwc(i["x"], i["packed"], Cout, k, stride, leaky, i.get("res"), out=o["y"]), ins,
                          {"y": ((B, Ho, Wo, Cout), torch.float32)}, device=gpu_device)
    tol = 4 * float(np.abs(yard - want).max())
    err = float(np.abs(outs["y"].cpu().numpy().astype(np.float64) - want).max())
    measured("det conv " + "x".join(str(int(v)) for v in case), err, tol)
    assert err <= tol, (err, tol)


# ---- 7. the handle's own buffers between guards (POSERISK_FENCE; tests/test_internal_fence_gpu.py has the other handles) ---------
@pytest.mark.parametrize("mode", ("1", "2"), ids=("head", "tail"))
def test_the_handles_buffers_stay_inside_their_guards(gpu_device, monkeypatch, mode):
    """Activations, packed weights, canvas and candidate list lie between 0xFF guards; B below max_batch, so that in tail mode every
    tensor ends on its buffer's end instead of starting on its start.  The bits are those of the unfenced handle."""
    lib = detector._lib.load()
    plain = _detector(gpu_device, dc.DETECT_SIZE)
    frames = torch.from_numpy(dc.frames(dc.DETECT_SEED, 2, *dc.DETECT_FRAME)).to(gpu_device)
    want = [t.clone() for t in plain.detect_raw(frames, False, dc.CONF, dc.NMS, 64)]
    x = plain.letterbox(frames)
    want86 = plain.network_until(x, 86).clone()
    monkeypatch.setenv("POSERISK_FENCE", mode)
    fenced = detector.Detector(dc.weights(), img_size=dc.DETECT_SIZE, device=gpu_device, max_batch=3)
    monkeypatch.delenv("POSERISK_FENCE")
    try:
        names = C.create_string_buffer(1 << 16)
        assert lib.pr_fence_list(names, len(names)) >= 4 and b"det act[0]" in names.value and b"det packed weights" in names.value
        got = fenced.detect_raw(frames, False, dc.CONF, dc.NMS, 64)
        got86 = fenced.network_until(x, 86)
        report = C.create_string_buffer(1 << 16)
        assert lib.pr_fence_check(report, len(report)) == 0, report.value.decode()
        for g, w in zip(got, want):
            assert torch.equal(g, w)
        assert torch.equal(got86, want86)
    finally:
        fenced.close()
    report = C.create_string_buffer(1 << 16)
    assert lib.pr_fence_check(report, len(report)) == 0, report.value.decode()
