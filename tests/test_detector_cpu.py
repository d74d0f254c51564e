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
