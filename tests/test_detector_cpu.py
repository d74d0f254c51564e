"""The person detector without a GPU: the topology table (the library's own against the facts of darknet's yolov3.cfg and
against the pure-Python table), the darknet file reader's refusals, the synthetic weights, the letterbox sizes, and the numpy
references' own sanity (tests/det_ref.py)."""
import numpy as np
import pytest

import det_cases as dc
import det_ref
from poserisk_release_amd import detector
from poserisk_release_amd.detector import CONV, ROUTE, SHORTCUT, UPSAMPLE, YOLO


def test_topology_holds_the_facts_of_yolov3_cfg():
    t = detector.topology()
    assert len(t) == 107
    count = lambda k: sum(l["type"] == k for l in t)
    assert (count(CONV), count(SHORTCUT), count(ROUTE), count(UPSAMPLE), count(YOLO)) == (75, 23, 4, 2, 3)
    routes = [(i, l["from0"], l["from1"]) for i, l in enumerate(t) if l["type"] == ROUTE]
    assert routes == [(83, 79, -1), (86, 85, 61), (95, 91, -1), (98, 97, 36)]            # -4 | -1,61 | -4 | -1,36
    assert [(i, l["down"]) for i, l in enumerate(t) if l["type"] == YOLO] == [(82, 32), (94, 16), (106, 8)]
    assert all(l["from0"] == i - 3 for i, l in enumerate(t) if l["type"] == SHORTCUT)
    heads = [l for l in t if l["type"] == CONV and not l["bn"]]
    assert [(l["cout"], l["ksize"]) for l in heads] == [(255, 1)] * 3 and [i for i, l in enumerate(t) if l["type"] == CONV and not l["bn"]] == [81, 93, 105]
    assert t[0]["cin"] == 3 and t[0]["cin_pad"] == 4 and t[0]["kpad"] == 64 and t[81]["cout_pad"] == 256
    assert {l["cin"] for l in t if l["type"] == CONV} >= {3, 32, 64, 128, 256, 384, 512, 768, 1024}
    lib = detector._lib.load()
    assert lib.pr_det_weight_floats(107) == detector.WEIGHT_FLOATS == 62001757 == detector.weight_floats()
    # offsets: consecutive in both layouts
    w = p = 0
    for l in t:
        if l["type"] == CONV:
            assert (l["weight_offset"], l["pack_offset"]) == (w, p)
            w += l["cout"] * (4 if l["bn"] else 1) + l["cout"] * l["cin"] * l["ksize"] ** 2
            p += l["cout_pad"] * (1 + l["kpad"])
        else:
            assert l["weight_offset"] == l["pack_offset"] == -1
    assert p == lib.pr_det_packed_floats(107)
    assert detector.ANCHORS == ((10, 13), (16, 30), (33, 23), (30, 61), (62, 45), (59, 119), (116, 90), (156, 198), (373, 326))
    assert detector.ANCHOR_MASKS == ((6, 7, 8), (3, 4, 5), (0, 1, 2))


def test_library_table_equals_the_python_table_and_truncates():
    py = detector.yolo_layers()
    for n in (1, 12, 107):
        t = detector.topology(n)
        assert len(t) == n
        for a, b in zip(t, py):
            got = (a["type"], a["cin"], a["cout"], a["ksize"], a["stride"], a["bn"], a["down"], tuple(x for x in (a["from0"], a["from1"]) if x >= 0))
            assert got == (b["type"], b["cin"], b["cout"], b["ksize"], b["stride"], b["bn"], b["down"], tuple(b["from"]))
    with pytest.raises(detector._lib.PoseRiskHipError, match="n_layers = 108"):
        detector.topology(108)


def test_the_shipped_library_folds_and_packs_like_numpy_float64():
    """The same comparison tests/test_detector_native.py makes on the sanitizer build, on the library Python loads, with darknet's
    epsilon as well as the default."""
    layers = detector.yolo_layers()[:9]
    rng = np.random.default_rng(6)
    body = rng.normal(0, 1, detector.weight_floats(layers)).astype(np.float32)
    p = 0
    for l in layers:
        if l["type"] == CONV:
            body[p + 3 * l["cout"]:p + 4 * l["cout"]] = rng.uniform(0.5, 1.5, l["cout"])
            p += 4 * l["cout"] + l["cout"] * l["cin"] * l["ksize"] ** 2
    for eps in (1e-5, 1e-6):
        want, used = det_ref.numpy_fold_pack(body, layers, eps)
        got = detector.fold_pack(body, n_layers=9, bn_eps=eps)
        assert used == body.size and np.array_equal(got.view(np.uint32), want.view(np.uint32)), eps
    with pytest.raises(detector._lib.PoseRiskHipError, match="n_floats"):
        detector.fold_pack(body[:-1], n_layers=9)


def test_load_darknet_reads_both_headers_and_refuses_by_name(tmp_path):
    body = np.arange(detector.WEIGHT_FLOATS, dtype=np.float32)
    for version in ((0, 2, 0), (0, 1, 0)):
        path = tmp_path / f"v{version[1]}.weights"
        detector.save_darknet(path, body, version=version, seen=32013312)
        assert path.stat().st_size == 4 * body.size + (20 if version[1] >= 2 else 16)
        assert np.array_equal(detector.load_darknet(str(path)), body)
    short = tmp_path / "short.weights"
    detector.save_darknet(short, body[:-3])
    with pytest.raises(ValueError, match=r"holds 6\.20018e\+07 floats, YOLOv3 with 80 classes holds 62001757"):
        detector.load_darknet(str(short))
    tiny = tmp_path / "tiny.weights"
    tiny.write_bytes(b"\0" * 10)
    with pytest.raises(ValueError, match="10 bytes are no darknet weight file"):
        detector.load_darknet(str(tiny))
    bad = tmp_path / "bad.weights"
    bad.write_bytes(np.asarray([-7, 2, 0], "<i4").tobytes() + b"\0" * 64)
    with pytest.raises(ValueError, match="bad darknet header"):
        detector.load_darknet(str(bad))


def test_synthetic_weights_have_the_file_layout():
    w = dc.weights()
    assert w.dtype == np.float32 and w.size == detector.WEIGHT_FLOATS and np.isfinite(w).all()
    params, used = det_ref.split_weights(w)
    assert used == w.size and len(params) == 75
    assert (params[0]["var"] > 0).all() and np.array_equal(params[0]["gamma"], np.ones(32, np.float32))
    bias = params[81]["bias"].reshape(3, 85)
    assert (bias[:, 4] == -3).all() and (bias[:, 5] == 3).all() and (bias[:, 6:] == -1).all() and not bias[:, :4].any()


def test_letterbox_sizes_follow_the_integer_rule():
    g = detector.letterbox_geometry
    assert g(54, 96, 64, 96) == (54, 96, 0, 5)
    assert g(450, 800, 416, 416) == (234, 416, 0, 91)
    assert g(450, 800, 256, 416) == (234, 416, 0, 11)
    assert g(97, 41, 64, 96) == (64, 27, 34, 0)             # 41 * 64 / 97 = 27.05
    assert g(23, 31, 64, 96) == (64, 86, 5, 0)              # enlarged: 31 * 64 / 23 = 86.26
    assert g(1, 4096, 32, 32) == (1, 32, 0, 15)             # never below one row
    assert g(3, 2, 32, 32) == (32, 21, 5, 0)                # 2 * 32 / 3 = 21.33
    assert g(2, 3, 32, 32)[:2] == (21, 32)
    assert g(5, 2, 32, 32)[:2] == (32, 13)                  # 12.8 rounds up; 2.5 -> 3 is round-half-up:
    assert g(64, 5, 32, 32)[:2] == (32, 3)                  # 5 * 32 / 64 = 2.5


def test_reference_letterbox_and_nms_are_sane():
    frames = dc.frames(1, 2, 54, 96)
    x = det_ref.letterbox(frames, 64, 96)
    assert x.shape == (2, 64, 96, 4) and not x[..., 3].any()
    assert np.array_equal(x[:, 5:59, :, :3], frames.astype(np.float32) * np.float32(1 / 255))        # same width, same height: a copy
    assert (x[:, :5, :, :3] == np.float32(128) * np.float32(1 / 255)).all() and (x[:, 59:, :, :3] == x[0, 0, 0, 0]).all()
    heads = dc.crafted_heads(*dc.POST_SIZE)
    cells = det_ref.decode(heads)
    order, kept, overflow, _ = det_ref.select(cells[0], dc.CONF, dc.NMS)
    assert 60 < order.size <= 130 and 0 < kept.size < order.size and not overflow
    assert np.all(np.diff(cells[0]["score"][order]) <= 0)
    boxes = cells[0]["box"][kept]
    for i in range(len(kept)):
        assert not np.any(det_ref.iou(boxes[i], boxes[i + 1:]) > dc.NMS)
    order2, kept2, overflow2, _ = det_ref.select(cells[2], dc.CONF, dc.NMS)
    assert overflow2 and order2.size == detector.MAX_CAND
    assert det_ref.select(cells[1], dc.CONF, dc.NMS)[0].size == 0


# ---- the post-processing reference on the contract's edges: hand-derived numbers (tests/test_detector_gpu.py, section 3b) ---------
def _contract(cells, conf=0.1, nms=0.4):
    c = det_ref.decode(dc.edge_heads(cells), np.float64, np.float32)[0]
    return c, det_ref.select(c, conf, nms)


def test_reference_ious_of_the_crafted_cells_are_the_hand_derived_ones():
    c, _ = _contract({dc.EDGE_A: {}, dc.EDGE_B: {}, dc.EDGE_C: {}, dc.EDGE_B16: {}, dc.EDGE_ANCHOR_PAIR[0]: {}, dc.EDGE_ANCHOR_PAIR[1]: {}})
    box = lambda cell: c["box"][dc.flat_index(cell)]
    assert c["box"].dtype == np.float32 and c["score"].dtype == np.float32
    assert box(dc.EDGE_A).tolist() == [-42.0, 3.0, 74.0, 93.0] and box(dc.EDGE_B).tolist() == [-10.0, 3.0, 106.0, 93.0]
    assert box(dc.EDGE_B16).tolist() == [10.5, -19.5, 69.5, 99.5]
    assert c["score"][dc.flat_index(dc.EDGE_A)] == np.float32(0.25) and c["obj"][dc.flat_index(dc.EDGE_A)] == np.float32(0.5)
    iou = lambda p, q: det_ref.iou(box(p), box(q)[None])[0]
    assert iou(dc.EDGE_A, dc.EDGE_B) == dc.EDGE_IOU_1 == np.float32(7560) / np.float32(13320)
    assert iou(dc.EDGE_A, dc.EDGE_C) == dc.EDGE_IOU_2 == np.float32(4680) / np.float32(16200) and abs(float(dc.EDGE_IOU_2) - 0.289) < 1e-3
    assert iou(dc.EDGE_B, dc.EDGE_B16) == np.float32(5310) / np.float32(12151) > np.float32(0.4)
    assert iou(*dc.EDGE_ANCHOR_PAIR) == np.float32(1350) / np.float32(3270) > np.float32(0.4)


def test_reference_selection_on_the_edges():
    flat = dc.flat_index
    abc = {dc.EDGE_A: {"tc0": 0.0}, dc.EDGE_B: {"tc0": -1.0}, dc.EDGE_C: {"tc0": -2.0}}
    _, (order, kept, overflow, _) = _contract(abc)
    assert order.tolist() == [flat(dc.EDGE_A), flat(dc.EDGE_B), flat(dc.EDGE_C)] and not overflow
    assert kept.tolist() == [flat(dc.EDGE_A), flat(dc.EDGE_C)]              # B fell to A; C overlaps A by 0.289 only, and B was not kept
    # ties: the lower flat index first, whatever order the cells were named in, across heads and across anchors
    for first, second in ((dc.EDGE_A, dc.EDGE_B), (dc.EDGE_B, dc.EDGE_B16), dc.EDGE_ANCHOR_PAIR):
        assert flat(first) < flat(second)
        _, (order, kept, _, _) = _contract({second: {}, first: {}})
        assert order.tolist() == [flat(first), flat(second)] and kept.tolist() == [flat(first)]
        assert _contract({second: {}, first: {}}, nms=1.0)[1][1].tolist() == [flat(first), flat(second)]
    # strictly greater: at the IoU itself both stay, one ulp below it the later one goes
    two = {dc.EDGE_A: {"tc0": 0.0}, dc.EDGE_B: {"tc0": -1.0}}
    assert _contract(two, nms=float(dc.EDGE_IOU_1))[1][1].size == 2
    assert _contract(two, nms=float(np.nextafter(dc.EDGE_IOU_1, np.float32(0))))[1][1].size == 1
    # greater or equal: objectness 0.5 at conf_thres 0.5
    assert _contract({dc.EDGE_B: {}}, conf=0.5)[1][0].size == 1
    assert _contract({dc.EDGE_B: {}}, conf=float(np.nextafter(np.float32(0.5), np.float32(1))))[1][0].size == 0
    # 0 / 0 is no overlap
    hd, _, cy, cx = dc.EDGE_B
    empty = {"box": (0, 0, -200, -200), "tc0": -1.0}
    c, (order, kept, _, ious) = _contract({(hd, 0, cy, cx): empty, (hd, 1, cy, cx): empty}, nms=0.0)
    assert kept.size == 2 and np.isnan(ious[0, 1]) and c["box"][order[0]].tolist() == [48.0] * 4


def test_reference_takes_non_finite_cells_out_and_reports_them():
    flat = dc.flat_index(dc.EDGE_B)
    for spec, out, bit in (({"to": np.nan}, True, True), ({"tc0": np.nan}, True, True), ({"box": (0, 0, np.inf, 0)}, True, True),
                           ({"box": (0, 0, 89, 0)}, True, True), ({"box": (np.nan, 0, 0, 0)}, True, True), ({"box": (0, 0, 80, 0)}, False, False),
                           ({"to": -8.0, "box": (np.nan, 0, 0, 0)}, True, False)):       # below the threshold: no candidate, no bit
        heads = dc.edge_heads({dc.EDGE_B: spec, dc.EDGE_A: {}})
        for dtype in (np.float64, np.float32):
            c = det_ref.decode(heads, dtype)[0]
            cand, nonfinite = det_ref.candidates(c, 0.1)
            assert (not cand[flat]) == out and nonfinite == bit, (spec, dtype)
            assert det_ref.select(c, 0.1, 0.4)[0].tolist() == [dc.flat_index(dc.EDGE_A)] + ([] if out else [flat])
    # a NaN among the other classes never beats class 0
    heads = dc.edge_heads({dc.EDGE_B: {}})
    hd, a, cy, cx = dc.EDGE_B
    heads[hd][0, cy, cx, a * 85 + 5 + 7] = np.nan
    c = det_ref.decode(heads)[0]
    assert c["person"][flat]
    cand, nonfinite = det_ref.candidates(c, 0.1)
    assert cand[flat] and cand.sum() == 1 and not nonfinite


def test_cut_heads_hold_what_the_cut_tests_need():
    M = detector.MAX_CAND
    for n, tie in ((M, False), (M + 1, False), (M + 1, True)):
        heads, pick = dc.cut_heads(n, tie)
        c = det_ref.decode(heads, np.float64, np.float32)[0]
        order, kept, overflow, _ = det_ref.select(c, 0.1, 1.0)
        assert len(set(pick)) == n and det_ref.candidates(c, 0.1)[0].sum() == n and overflow == (n > M)
        assert order.size == M and np.array_equal(order, kept)
        s = np.sort(c["score"][[dc.flat_index(p) for p in pick]])
        assert (np.diff(s)[1 if tie else 0:] > 1e-5).all() and (s[0] == s[1]) == tie


def test_status_text_names_every_set_bit():
    texts = [detector.status_text(s, 0.1, 100) for s in range(8)]
    assert texts[0] == ""
    names = {detector.STATUS_CAND_OVERFLOW: "more than 1024 candidates above conf_thres 0.1", detector.STATUS_DET_OVERFLOW: "more than 100 boxes after NMS",
             detector.STATUS_NONFINITE: "not finite"}
    assert sorted(names) == [1, 2, 4]
    for s in range(8):
        for bit, name in names.items():
            assert (name in texts[s]) == bool(s & bit), (s, bit, texts[s])
        assert texts[s].count(";") == max(0, bin(s).count("1") - 1) and "unknown" not in texts[s]
    assert "unknown status bits 0x8" in detector.status_text(9, 0.1, 100) and "candidates" in detector.status_text(9, 0.1, 100)


def test_unmap_symbol_and_status_bit_are_declared_bound_and_exported():
    import os
    import re
    from conftest import REPO
    hdr = open(os.path.join(REPO, "include", "poserisk_hip.h")).read()
    lib = detector._lib.load()
    assert re.search(r"\bpr_det_unmap\s*\(", hdr) and "pr_det_unmap" in detector._lib.SIGNATURES and hasattr(lib, "pr_det_unmap")
    assert lib.pr_det_unmap.argtypes == detector._lib.SIGNATURES["pr_det_unmap"][1]
    assert re.search(r"PR_DET_STATUS_NONFINITE\s*=\s*4\b", hdr) and detector.STATUS_NONFINITE == 4
    assert lib.pr_abi_version() == detector._lib.ABI_VERSION      # a function was added: no ABI bump
    # refusals come before any device work: they need no GPU
    for args, name in (((None, 1, 2, 4, 54, 96, 64, 96), "null boxes_dev"), ((1, None, 2, 4, 54, 96, 64, 96), "null count_dev"),
                       ((1, 1, 4097, 4, 54, 96, 64, 96), "B = 4097"), ((1, 1, 2, 1025, 54, 96, 64, 96), "max_det = 1025"),
                       ((1, 1, 2, 4, 54, 0, 64, 96), "frames of 0 x 54"), ((1, 1, 2, 4, 54, 96, 64, 100), "multiples of 32")):
        with pytest.raises(detector._lib.PoseRiskHipError, match="pr_det_unmap: .*" + name):
            detector._lib.check(lib.pr_det_unmap(*args, None), "pr_det_unmap")
