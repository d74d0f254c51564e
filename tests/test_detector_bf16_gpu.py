"""The person detector in bf16 on the GPU (include/poserisk_hip.h, section j8, paragraph "bf16"), every tensor inside guard bands.

  a  the convolution alone (csrc/det_conv_bf16.hip) against a float64 evaluation of bf16-representable inputs
  b  the network, every checked layer from its OWN GPU inputs: the sharp test
  c  the network as a whole against float64, beside the emulation's error: guards against drift only
  d  plumbing: detect_raw against its own stages, refusals by name, the internal fence
  e  the Predictor with cfg.TRACKER.precision

Pass criterion of a and b, for a bf16 output g: bf16(v64 - t) <= g <= bf16(v64 + t), v64 the float64 value before the final
rounding and t = 4 x max |float32 torch evaluation - v64| on the same inputs -- the project's margin for another fp32 summation
order, and nothing more.  Rounding is monotonic, so this is exactly "the correctly rounded result of some value within t of the
exact one".  For an fp32 output: |g - v64| <= t.

c's caps (GPU rms <= 1.25 x emulation rms, GPU max <= 2 x emulation max, each against tests/det_ref.py's float64 forward) are
conditions, not measurements: emulations that take the same roundings the other way (float64, float32, float64 with 2e-6 relative
noise on every sum) lie within 0.94 - 1.05 of one another in rms and 0.67 - 1.28 in max on these tensors."""
import ctypes as C
import json
import sys
import types

import numpy as np
import pytest
import torch

import det_bf16_ref as br
import det_cases as dc
import det_ref
import guard_band as gb
from conftest import measured
from poserisk_release_amd import detector, ops, sort, synth, y4m
from test_detector_gpu import _net_ref

pytestmark = pytest.mark.gpu
_detectors = {}


def _detector(device, size, max_batch=3):
    key = (str(device), size, max_batch)
    if key not in _detectors:
        _detectors[key] = detector.Detector(dc.weights(), img_size=size, device=device, max_batch=max_batch, max_det=detector.MAX_CAND,
                                            precision="bf16")
    return _detectors[key]


def _to_bf16(a):
    """numpy f32 holding bf16 values -> a torch.bfloat16 CPU tensor of the same bits."""
    return torch.from_numpy(br.bf16_bits(a).view(np.int16).reshape(np.shape(a))).view(torch.bfloat16)


def _values(t):
    """A tensor from the GPU (bf16 or f32) -> numpy float64 of its values."""
    return t.detach().cpu().to(torch.float64).numpy()


# ---- a. the convolution alone -------------------------------------------------------------------------------------------------------
CONV_CASES = (          # (B, H, W, Cin, Cout, ksize, stride, leaky, residual, out)
    (2, 13, 17, 8, 32, 3, 1, True, False, "bf16"),
    (1, 13, 17, 32, 64, 3, 2, True, False, "bf16"),
    (3, 7, 9, 64, 128, 3, 1, True, True, "bf16"),
    (2, 5, 11, 768, 256, 1, 1, True, False, "bf16"),
    (2, 9, 7, 64, 255, 1, 1, False, False, "f32"),
    (2, 9, 7, 64, 255, 1, 1, True, False, "bf16"),
    (1, 3, 5, 40, 100, 3, 2, False, True, "bf16"),
    (1, 3, 5, 40, 30, 3, 1, True, True, "bf16"),
)


@pytest.mark.parametrize("case", CONV_CASES, ids=lambda c: "x".join(str(int(v)) if not isinstance(v, str) else v for v in c))
def test_det_conv_bf16_alone_against_float64(gpu_device, case):
    B, H, W, Cin, Cout, k, stride, leaky, with_res, out = case
    rng = np.random.default_rng(9)
    x = br.bf16_round(rng.standard_normal((B, H, W, Cin), dtype=np.float32)).reshape(B, H, W, Cin)
    w = br.bf16_round(rng.standard_normal((Cout, Cin, k, k), dtype=np.float32) * np.float32(np.sqrt(2.0 / (Cin * k * k)))).reshape(Cout, Cin, k, k)
    b = rng.standard_normal(Cout, dtype=np.float32)
    Ho, Wo = (H + 2 * (k // 2) - k) // stride + 1, (W + 2 * (k // 2) - k) // stride + 1
    res = br.bf16_round(rng.standard_normal((B, Ho, Wo, Cout), dtype=np.float32)).reshape(B, Ho, Wo, Cout) if with_res else None
    cout_pad, kpad = -(-Cout // 64) * 64, -(-(k * k * Cin) // 32) * 32
    packed = np.zeros((cout_pad, kpad), np.float32)
    packed[:Cout, :k * k * Cin] = w.transpose(0, 2, 3, 1).reshape(Cout, -1)
    bias = np.zeros(cout_pad, np.float32)
    bias[:Cout] = b
    blob = np.frombuffer(bias.tobytes() + br.bf16_bits(packed).tobytes(), np.uint8).copy()

    def ref(dt):
        y = torch.nn.functional.conv2d(torch.from_numpy(x).to(dt).permute(0, 3, 1, 2), torch.from_numpy(w).to(dt), torch.from_numpy(b).to(dt),
                                       stride=stride, padding=k // 2)
        if leaky:
            y = torch.nn.functional.leaky_relu(y, br.SLOPE)
        y = y.permute(0, 2, 3, 1)
        return (y + torch.from_numpy(res).to(dt) if with_res else y).to(torch.float64).numpy()

    v64, yard = ref(torch.float64), ref(torch.float32)
    t = 4 * float(np.abs(yard - v64).max())
    ins = {"x": _to_bf16(x), "packed": torch.from_numpy(blob)}
    if with_res:
        ins["res"] = _to_bf16(res)
    dt = torch.float32 if out == "f32" else torch.bfloat16
    outs = gb.run_guarded(lambda i, o: ops.det_conv_nhwc_bf16(i["x"], i["packed"], Cout, k, stride, leaky, i.get("res"), dt, out=o["y"]), ins,
                          {"y": ((B, Ho, Wo, Cout), dt)}, device=gpu_device)
    got = _values(outs["y"])
    name = "det bf16 conv " + "x".join(str(int(v)) if not isinstance(v, str) else v for v in case)
    measured(name + " band t", t)
    measured(name + " distance from float64" + ("" if out == "f32" else ", the final rounding included"), float(np.abs(got - v64).max()),
             t if out == "f32" else None)
    bad = br.band_failures(got, v64, t, out_f32=out == "f32")
    assert len(bad) == 0, f"{len(bad)} of {got.size} outside the band, first {bad[0].tolist()}: {got[tuple(bad[0])]!r} for {v64[tuple(bad[0])]!r} +- {t:.3e}"


# ---- b. the network, every checked layer from its own GPU inputs ------------------------------------------------------------------
CHECKED = (0, 1, 2, 3, 4, 36, 61, 74, 79, 81, 82, 84, 85, 86, 87, 93, 94, 97, 98, 105, 106)
_layers = detector.yolo_layers()
FETCHED = tuple(sorted(set(CHECKED) | {s for l in CHECKED for s in br.sources(l, _layers) if s >= 0}))
_runs = {}


def _run_network(device, size, B):
    """Every fetched layer through network_until and the heads through network, once per (size, B): {layer: tensor}, [heads]."""
    if (size, B) not in _runs:
        det = _detector(device, size)
        x = _net_ref(size)[0]
        shapes = {f"layer{l}": ((B,) + det.layer_shape(l), det.layer_dtype(l)) for l in FETCHED}
        shapes.update({f"head{i}": ((B, gh, gw, 255), torch.float32) for i, (gh, gw) in enumerate(det.grids)})

        def run(i, o):
            det.network(i["x"], out=[o["head0"], o["head1"], o["head2"]])
            for l in FETCHED:
                det.network_until(i["x"], l, out=o[f"layer{l}"])

        outs = gb.run_guarded(run, {"x": torch.from_numpy(x[:B])}, shapes, device=device)
        _runs[(size, B)] = ({l: outs[f"layer{l}"].clone() for l in FETCHED}, [outs[f"head{i}"].clone() for i in range(3)])
    return _runs[(size, B)]


@pytest.mark.parametrize("B", dc.NETWORK_BATCHES)
@pytest.mark.parametrize("size", dc.NETWORK_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_network_layers_from_their_own_gpu_inputs(gpu_device, size, B):
    det = _detector(gpu_device, size)
    assert det.precision == "bf16" and detector._lib.load().pr_det_precision(det._h) == 1
    layers, heads = _run_network(gpu_device, size, B)
    for l in FETCHED:
        want = torch.float32 if l in br.FP32_LAYERS else torch.bfloat16
        assert det.layer_dtype(l) == want == layers[l].dtype, l
    inputs = {l: _values(t) for l, t in layers.items()}
    inputs[-1] = _net_ref(size)[0][:B]
    failures = []
    for l in CHECKED:
        try:
            err, t = br.check_layer(l, inputs[l], inputs)
            if t:      # a convolution or a fused shortcut; for a bf16 tensor the distance includes its own final rounding
                measured(f"det bf16 {size[0]}x{size[1]} B{B} layer{l} from its inputs: band t", t)
                measured(f"det bf16 {size[0]}x{size[1]} B{B} layer{l} from its inputs: distance", err, t if l in br.FP32_LAYERS else None)
        except AssertionError as e:
            failures.append(str(e))
    # the heads through pr_det_network are the bits of the yolo layers through pr_det_network_until
    for i, h in enumerate(detector.HEAD_LAYERS):
        assert torch.equal(heads[i], layers[h]), h
    # a frame's bits do not depend on its batch
    if B > 1:
        one, heads1 = _run_network(gpu_device, size, 1)
        for l in FETCHED:
            assert torch.equal(layers[l][:1].view(torch.uint8), one[l].view(torch.uint8)), f"layer {l}: frame 0 of B = {B} is not the B = 1 run"
        for a, b in zip(heads, heads1):
            assert torch.equal(a[:1], b)
    assert not failures, failures


# ---- c. the network as a whole, against float64 -------------------------------------------------------------------------------------
WHOLE = (82, 94, 106, 36, 61, 98)
_emulations = {}


def _emulation(size):
    if size not in _emulations:
        _emulations[size] = br.forward(dc.weights(), _net_ref(size)[0], torch.float64)
    return _emulations[size]


@pytest.mark.parametrize("size", dc.NETWORK_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_network_error_against_float64_stays_at_the_emulations(gpu_device, size):
    B = 3
    layers, _ = _run_network(gpu_device, size, B)
    ref64, emu = _net_ref(size)[1], _emulation(size)
    failures = []
    for l in WHOLE:
        want = ref64[l][:B].astype(np.float64)
        eg, ee = _values(layers[l]) - want, emu[l][:B] - want
        g_rms, e_rms = float(np.sqrt(np.mean(eg ** 2))), float(np.sqrt(np.mean(ee ** 2)))
        g_max, e_max = float(np.abs(eg).max()), float(np.abs(ee).max())
        tag = f"det bf16 {size[0]}x{size[1]} layer{l}"
        measured(f"{tag} emulation rms", e_rms)
        measured(f"{tag} gpu rms", g_rms, 1.25 * e_rms)
        measured(f"{tag} emulation max", e_max)
        measured(f"{tag} gpu max", g_max, 2 * e_max)
        measured(f"{tag} tensor rms", float(np.sqrt(np.mean(want ** 2))))
        if not (g_rms <= 1.25 * e_rms and g_max <= 2 * e_max):
            failures.append(f"layer {l}: rms {g_rms:.3e} against 1.25 x {e_rms:.3e}, max {g_max:.3e} against 2 x {e_max:.3e}")
    assert not failures, failures


# ---- d. plumbing --------------------------------------------------------------------------------------------------------------------
def test_detect_raw_equals_its_own_stages(gpu_device):
    S_h, S_w = dc.DETECT_SIZE
    H, W = dc.DETECT_FRAME
    B, M = 3, 256
    det = _detector(gpu_device, dc.DETECT_SIZE)
    frames = dc.frames(dc.DETECT_SEED, B, H, W)
    outs = gb.run_guarded(lambda i, o: det.detect_raw(i["frames"], False, dc.CONF, dc.NMS, M, out=o), {"frames": torch.from_numpy(frames)},
                          {"boxes": ((B, M, 4), torch.float32), "scores": ((B, M), torch.float32), "count": ((B,), torch.int32),
                           "status": ((B,), torch.int32)}, device=gpu_device)
    dev_frames = torch.from_numpy(frames).to(gpu_device)
    lb_boxes, lb_scores, lb_count, lb_status = det.postprocess(det.network(det.letterbox(dev_frames)), dc.CONF, dc.NMS, M)
    assert torch.equal(outs["count"], lb_count) and torch.equal(outs["status"], lb_status) and torch.equal(outs["scores"], lb_scores)
    assert int(lb_count.sum()) > 0
    boxes, lb = outs["boxes"].cpu().numpy(), lb_boxes.cpu().numpy()
    for b in range(B):
        n = int(lb_count[b])
        if n:
            want = det_ref.unmap(lb[b, :n], H, W, S_h, S_w, np.float64)
            tol = 4 * float(np.abs(det_ref.unmap(lb[b, :n], H, W, S_h, S_w, np.float32).astype(np.float64) - want).max())
            err = float(np.abs(boxes[b, :n].astype(np.float64) - want).max())
            measured(f"det bf16 detect frame {b} unmap", err, tol, "px")
            assert err <= tol, (b, err, tol)
        assert not boxes[b, n:].any()


def test_bf16_entries_refuse_by_name(gpu_device):
    lib = detector._lib.load()
    body = np.ascontiguousarray(dc.weights(), np.float32)
    h = C.c_void_p()
    st = lib.pr_det_create_p(gpu_device.index, body.ctypes.data_as(C.c_void_p), body.size, 32, 64, 1, 1e-5, 2, C.byref(h))
    with pytest.raises(detector._lib.PoseRiskHipError, match="precision = 2, must be 0 \\(fp32\\) or 1 \\(bf16\\)"):
        detector._lib.check(st, "pr_det_create_p")
    assert not h.value
    det = _detector(gpu_device, (32, 64))
    x = torch.zeros((4, 32, 64, 4), device=gpu_device)
    with pytest.raises(detector._lib.PoseRiskHipError, match="max_batch = 3"):
        det.network(x)
    with pytest.raises(detector._lib.PoseRiskHipError, match="max_batch = 3"):
        det.network_until(x, 5)
    xb = torch.zeros((1, 4, 4, 12), dtype=torch.bfloat16, device=gpu_device)
    with pytest.raises(detector._lib.PoseRiskHipError, match="Cin = 12, must be a multiple of 8"):
        ops.det_conv_nhwc_bf16(xb, torch.zeros(64 * 4 + 64 * 32 * 2, dtype=torch.uint8, device=gpu_device), 8, 1)
    with pytest.raises(ValueError, match="one of 'fp32', 'bf16'"):
        detector.Detector(dc.weights(), img_size=(32, 64), device=gpu_device, precision="fp16")


@pytest.mark.parametrize("mode", ("1", "2"), ids=("head", "tail"))
def test_the_bf16_handles_buffers_stay_inside_their_guards(gpu_device, monkeypatch, mode):
    """B below max_batch, so that in tail mode every tensor ends on its buffer's end; the bits are the unfenced handle's."""
    lib = detector._lib.load()
    plain = _detector(gpu_device, dc.DETECT_SIZE)
    frames = torch.from_numpy(dc.frames(dc.DETECT_SEED, 2, *dc.DETECT_FRAME)).to(gpu_device)
    want = [t.clone() for t in plain.detect_raw(frames, False, dc.CONF, dc.NMS, 64)]
    x = plain.letterbox(frames)
    want86, want81 = plain.network_until(x, 86).clone(), plain.network_until(x, 81).clone()
    monkeypatch.setenv("POSERISK_FENCE", mode)
    fenced = detector.Detector(dc.weights(), img_size=dc.DETECT_SIZE, device=gpu_device, max_batch=3, precision="bf16")
    monkeypatch.delenv("POSERISK_FENCE")
    try:
        names = C.create_string_buffer(1 << 16)
        assert lib.pr_fence_list(names, len(names)) >= 4 and b"det act[0]" in names.value and b"det packed weights" in names.value
        got = fenced.detect_raw(frames, False, dc.CONF, dc.NMS, 64)
        got86, got81 = fenced.network_until(x, 86), fenced.network_until(x, 81)
        torch.cuda.synchronize()
        report = C.create_string_buffer(1 << 16)
        assert lib.pr_fence_check(report, len(report)) == 0, report.value.decode()
        for g, w in zip(got, want):
            assert torch.equal(g, w)
        assert got86.dtype == torch.bfloat16 and torch.equal(got86.view(torch.int16), want86.view(torch.int16)) and torch.equal(got81, want81)
    finally:
        fenced.close()
    report = C.create_string_buffer(1 << 16)
    assert lib.pr_fence_check(report, len(report)) == 0, report.value.decode()


# ---- e. the Predictor ---------------------------------------------------------------------------------------------------------------
def test_predictor_tracks_with_the_bf16_detector(gpu_device, tmp_path, monkeypatch):
    from poserisk_release_amd import dropin
    dropin.install()
    from core import base
    from core.config import cfg
    from models import hmr
    from smpl import SMPL
    monkeypatch.setitem(sys.modules, "cv2", None)
    monkeypatch.setitem(sys.modules, "multi_person_tracker", None)
    weight_file = str(tmp_path / "synthetic.weights")
    detector.save_darknet(weight_file, dc.weights())
    W, H, n = 320, 180, 8          # the clip of test_predictor_tracks_with_the_built_in_detector
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
    assert cfg.TRACKER.precision == "fp32"
    monkeypatch.setitem(cfg.TRACKER, "weights", weight_file)
    monkeypatch.setitem(cfg.TRACKER, "img_size", (64, 96))
    monkeypatch.setitem(cfg.TRACKER, "batch", 3)
    decoded = y4m.decode(str(clip), gpu_device)

    def same(a, b):
        assert list(a) == list(b)
        for k in b:
            assert np.array_equal(a[k]["bbox"], b[k]["bbox"]) and np.array_equal(a[k]["frames"], b[k]["frames"]), k

    # the knob at its default: today's tracking, bit for bit
    today = sort.track_frames(detector.Detector(weight_file, img_size=(64, 96), device=gpu_device, max_batch=3).detect(decoded, conf_thres=0.1,
                                                                                                                      nms_thres=0.4))
    same(pred.track_frames(decoded), today)
    assert pred._detector.precision == "fp32"
    monkeypatch.setitem(cfg.TRACKER, "precision", "bf16")
    out = pred(str(clip), str(tmp_path / "info.json"), str(tmp_path / "out"))
    assert pred._detector.precision == "bf16"          # the precision is part of the cache key: the fp32 handle was replaced
    dets = detector.Detector(weight_file, img_size=(64, 96), device=gpu_device, max_batch=3, precision="bf16").detect(decoded, conf_thres=0.1,
                                                                                                                     nms_thres=0.4)
    tracking = sort.track_frames(dets)
    assert tracking and max(len(t["frames"]) for t in tracking.values()) >= 3
    same(pred.track_frames(decoded), tracking)
    want = pred.score_frames(decoded, tracking, synth.EXAMPLE_INFO)
    assert len(out["frames"]) >= 3
    for k in ("result", "joint_cam", "frames"):
        assert np.array_equal(np.asarray(out[k]), np.asarray(want[k])), k
    for t in ("reba", "rula"):
        np.testing.assert_array_equal(np.asarray(out[t][0], np.float64), np.asarray(want[t][0], np.float64), err_msg=t)
    monkeypatch.setitem(cfg.TRACKER, "precision", "fp32")
    same(pred.track_frames(decoded), today)
    # the comparison a holder of real weights runs: every box of either precision is counted once, and the totals are the rows' sums
    lines = []
    fp32_dets = detector.Detector(weight_file, img_size=(64, 96), device=gpu_device, max_batch=3).detect(decoded, conf_thres=0.1, nms_thres=0.4)
    rows, total = detector.compare(weight_file, decoded, img_size=(64, 96), device=gpu_device, batch=3, report=lines.append)
    assert len(rows) == n and len(lines) == n + 1 and lines[-1].startswith(f"total over {n} frames: both {total['both']}")
    for r, a, b in zip(rows, fp32_dets, dets):
        assert r["both"] + r["fp32_only"] == len(a) and r["both"] + r["bf16_only"] == len(b), r
    assert total["both"] == sum(r["both"] for r in rows) > 0
    monkeypatch.setitem(cfg.TRACKER, "precision", "fp16")
    with pytest.raises(ValueError, match="'fp16' unknown: one of 'fp32', 'bf16'"):
        pred.track_frames(decoded)
