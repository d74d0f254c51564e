"""The crop kernel on the knife edges of its contract (tests/crop_cases.py): every box whose crop depends on the order of
the double roundings, the frames and boxes the random tests never reach, and the boxes that have no crop at all -- bit for
bit against oracle/crop_ref.py, status included."""
import ctypes as C

import numpy as np
import pytest
import torch

import crop_cases as cc
from conftest import measured
from oracle import crop_ref
from poserisk_release_amd import _lib, ops

pytestmark = pytest.mark.gpu

F = 2


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


@pytest.fixture(scope="module")
def frames():
    return np.random.default_rng(12).integers(0, 256, (F, cc.FRAME_H, cc.FRAME_W, 3), dtype=np.uint8)


@pytest.fixture(scope="module")
def knife_edges(frames):
    """[(family, scale, boxes, frame index, the oracle's crops)], the oracle run once for all tests here."""
    out = []
    for fam, scale, boxes in cc.selected():
        idx = (np.arange(len(boxes)) % F).astype(np.int32)
        want = np.stack([crop_ref.crop_to_tensor(frames[i], b, scale) for i, b in zip(idx, boxes)])
        out.append((fam, scale, boxes, idx, want))
    return out


def test_knife_edge_boxes_bit_exact(gpu_device, frames, knife_edges):
    """Every selected box, none sampled: a kernel that contracts `112 - a sx0`, `112 - d sy0` or `M4 y + M5` into a fused
    multiply-add differs from the oracle on each of them (tests/test_crop_edges_cpu.py proves that in emulation)."""
    d_rgb, d_bgr = _t(frames, gpu_device), _t(frames[..., ::-1], gpu_device)
    bad, total = {}, 0
    for fam, scale, boxes, idx, want in knife_edges:
        got = ops.crop_frames(d_rgb, boxes, idx, scale=scale).cpu().numpy()
        got_bgr = ops.crop_frames(d_bgr, boxes, idx, scale=scale, bgr=True).cpu().numpy()
        assert np.array_equal(got_bgr, got), (fam, scale)
        wrong = [i for i in range(len(boxes)) if not np.array_equal(got[i], want[i])]
        total += len(boxes)
        if wrong:
            bad[(fam, scale)] = wrong
        measured(f"crop_edges.gpu.{fam}.scale{scale:g}.boxes_that_differ", len(wrong))
    measured("crop_edges.gpu.boxes", total)
    measured("crop_edges.gpu.boxes_that_differ", sum(len(v) for v in bad.values()))
    assert not bad, {k: (len(v), v[:4]) for k, v in bad.items()}


def test_scale_is_the_double_the_reference_multiplies_by(gpu_device, frames):
    """Ordinary boxes whose crop differs between scale 1.2 and the float32 nearest to it (which is what crosses the C entry):
    the kernel gives the double's crop, bit for bit."""
    boxes, _ = cc.scale_width_boxes()
    idx = (np.arange(len(boxes)) % F).astype(np.int32)
    got = ops.crop_frames(_t(frames, gpu_device), boxes, idx, scale=1.2).cpu().numpy()
    wrong = [i for i in range(len(boxes)) if not np.array_equal(got[i], crop_ref.crop_to_tensor(frames[idx[i]], boxes[i], 1.2))]
    measured("crop_edges.gpu.scale_width.boxes_that_differ", len(wrong))
    assert not wrong, (wrong, boxes[wrong[:4]])
    # a scale with more digits than a float32 holds is still the float32 it was rounded to, read as its shortest decimal
    s = 1.23456789
    short = float(np.format_float_positional(np.float32(s), unique=True))
    assert short == 1.2345679
    got = ops.crop_frames(_t(frames, gpu_device), boxes[:4], idx[:4], scale=s).cpu().numpy()
    for i in range(4):
        np.testing.assert_array_equal(got[i], crop_ref.crop_to_tensor(frames[idx[i]], boxes[i], short))


@pytest.mark.parametrize("hw", [(1, 1), (1, 2), (2, 1)])
def test_tiny_frames_bit_exact(gpu_device, hw):
    """Frames too small for the 8-byte row load: every tap goes through the byte path and the border zeros."""
    H, W = hw
    fr = np.random.default_rng(13).integers(1, 256, (F, H, W, 3), dtype=np.uint8)
    boxes = np.array([[0.0, 0.0, 2.0, 2.0], [0.3, 0.4, 1.0, 3.0], [0.5, 0.5, 6.0, 5.0], [W - 1.0, H - 1.0, 0.75, 0.75],
                      [-0.5, 0.25, 300.0, 280.0], [0.0, 0.0, -2.0, 2.0]], np.float32)
    idx = (np.arange(len(boxes)) % F).astype(np.int32)
    got, status = ops.crop_frames(_t(fr, gpu_device), boxes, idx, return_status=True)
    assert status.cpu().tolist() == [0] * len(boxes)
    got = got.cpu().numpy()
    for n, box in enumerate(boxes):
        np.testing.assert_array_equal(got[n], crop_ref.crop_to_tensor(fr[idx[n]], box, 1.2), err_msg=f"{hw} box {n}")
    assert got.max() > 0


def test_last_byte_of_the_last_frame_and_far_away_boxes(gpu_device, frames):
    """Crop pixel (223, 223) of a 1:1 box (scale 1, side 224) reads source pixel (cx + 111, cy + 111) and its right and lower
    neighbours: with the neighbours on the last column and row of the LAST frame the tap ends on the buffer's last byte, where
    the kernel must leave its 8-byte load.  A box 2^17 pixels off the frame reads nothing: zeros, and no status bit."""
    H, W = cc.FRAME_H, cc.FRAME_W
    far = float(1 << 17)
    boxes = np.array([[W - 2 - 111, H - 2 - 111, 224, 224],            # integer positions: weight (32767, 0, 0, 1)
                      [W - 2 - 111 + 0.5, H - 2 - 111 + 0.5, 224, 224],    # half-way: the last pixel carries a quarter
                      [W - 2 - 111 + 31 / 32, H - 2 - 111 + 31 / 32, 224, 224],
                      [W + far, 100.0, 60.0, 90.0], [100.0, -far, 60.0, 90.0], [-far, H + far, 224, 224]], np.float32)
    scale = 1.0
    e = cc.emulate(boxes[1], scale, False)
    assert ((e[0] + e[2][223]) >> 10, (e[1][223] + e[3][223]) >> 10) == (W - 2, H - 2)
    idx = np.full(len(boxes), F - 1, np.int32)
    got, status = ops.crop_frames(_t(frames, gpu_device), boxes, idx, scale=scale, return_status=True)
    got = got.cpu().numpy()
    assert status.cpu().tolist() == [0] * len(boxes)
    for n, box in enumerate(boxes):
        np.testing.assert_array_equal(got[n], crop_ref.crop_to_tensor(frames[F - 1], box, scale), err_msg=f"box {n}")
    assert got[1, :, 223, 223].max() > 0 and not got[3:].any()
    assert got[1, 0, 223, 223] == np.float32(
        (int(frames[F - 1, H - 2:, W - 2:, 0].astype(np.int64).sum()) * 8192 + (1 << 14)) >> 15) / np.float32(255)


# ---------------------------------------------------------------------------------------------------------------------
# boxes without a defined crop: status bit 1, zeros
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", [1.2, 1.0])
def test_refused_boxes_status_and_zeros(gpu_device, frames, scale):
    table = cc.status_table(scale)
    boxes = np.stack([b for _, b, _ in table])
    idx = (np.arange(len(boxes)) % F).astype(np.int32)
    with np.errstate(all="ignore"):
        want_status = [crop_ref.box_status(b, scale) for b in boxes]
        want = np.stack([crop_ref.crop_to_tensor(frames[i], b, scale) for i, b in zip(idx, boxes)])
    assert want_status == [w for _, _, w in table]
    out = torch.full((len(boxes), 3, 224, 224), 7.0, device=gpu_device)
    st = torch.full((len(boxes),), -1, dtype=torch.int32, device=gpu_device)
    got, status = ops.crop_frames(_t(frames, gpu_device), boxes, idx, scale=scale, return_status=True, out=(out, st))
    status, got = status.cpu().tolist(), got.cpu().numpy()
    wrong = [(table[i][0], status[i], want_status[i]) for i in range(len(table)) if status[i] != want_status[i]]
    assert not wrong, wrong
    for i, (name, _, w) in enumerate(table):
        np.testing.assert_array_equal(got[i], want[i], err_msg=name)
        assert w == 0 or not got[i].any(), name
    # the accepted neighbours of the refused boxes are real crops: a side one float32 past absorption still reads the frame
    on_frame = ("good", "w_not_absorbed_at_0.5", "h_not_absorbed_at_0.5", "w_not_absorbed_at_300", "w_negative", "h_negative")
    assert all(got[i].any() for i, (name, _, _) in enumerate(table) if name in on_frame)


def test_refused_box_leaves_its_neighbours_alone_and_both_bits_can_be_set(gpu_device, frames):
    good = np.array([[100.25, 80.5, 60.0, 90.0], [200.0, 120.0, 150.0, 100.0]], np.float32)
    refused = [[100.0, 80.0, 0.0, 50.0], [float("nan"), 80.0, 30.0, 50.0], [100.0, 80.0, 30.0, float("inf")],
               [3e5, 80.0, 30.0, 50.0]]
    d = _t(frames, gpu_device)
    alone = ops.crop_frames(d, good, np.array([0, 1], np.int32)).cpu().numpy()
    for r in refused:
        boxes = np.array([good[0], r, good[1]], np.float32)
        crops, status = ops.crop_frames(d, boxes, np.array([0, 1, 1], np.int32), return_status=True)
        assert status.cpu().tolist() == [0, 2, 0], r
        crops = crops.cpu().numpy()
        assert np.array_equal(crops[0], alone[0]) and np.array_equal(crops[2], alone[1]) and not crops[1].any(), r
    # a refused box on a frame that does not exist: both bits; a good box there: bit 0 alone
    idx = torch.tensor([0, 5, -1, 1], dtype=torch.int32, device=gpu_device)
    boxes = np.array([good[0], refused[0], good[1], refused[1]], np.float32)
    crops, status = ops.crop_frames(d, boxes, idx, return_status=True)
    assert status.cpu().tolist() == [0, 3, 1, 2]
    assert not crops[1:].cpu().numpy().any() and np.array_equal(crops[0].cpu().numpy(), alone[0])
    # through the C entry without a status pointer: refused crops are still zeros, the others their usual bits
    out = torch.full((4, 3, 224, 224), 5.0, device=gpu_device)
    bb = _t(boxes, gpu_device)
    rc = _lib.load().pr_crop_frames(d.data_ptr(), F, cc.FRAME_H, cc.FRAME_W, 0, idx.data_ptr(), bb.data_ptr(), 4,
                                    C.c_float(1.2), out.data_ptr(), None, None)
    torch.cuda.synchronize()
    assert rc == 0 and torch.equal(out, crops)


def test_frame_feed_flags_a_refused_box(gpu_device):
    """One FrameFeed batch with one refused box: bit 1 in that row's crop_status, and the rows around it carry the bits they
    carry when a good box stands in its place."""
    from poserisk_release_amd import synth
    from poserisk_release_amd.feed import FrameFeed
    from poserisk_release_amd.hmr import HMR
    from poserisk_release_amd.pipeline import FramePipeline
    from poserisk_release_amd.smpl_layer import SMPLLayer
    B, H, W = 4, 120, 160
    rng = np.random.default_rng(14)
    fr = rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)
    boxes = np.stack([rng.uniform(40, 120, B), rng.uniform(30, 90, B), rng.uniform(30, 80, B), rng.uniform(40, 100, B)],
                     1).astype(np.float32)
    with_refused = boxes.copy()
    with_refused[2, 2] = 0.0
    m = HMR(max_batch=B).to(gpu_device)
    m.load_state_dict(synth.hmr_state_dict(seed=1))
    pipe = FramePipeline(m, SMPLLayer(synth.smpl_model(V=6890, seed=2), device=gpu_device, max_batch=16), synth.EXAMPLE_INFO)
    feed = FrameFeed(pipe, B, (H, W), gpu_device)
    usual, flagged = list(feed.run([(fr, boxes), (fr, with_refused)]))
    assert usual["crop_status"].tolist() == [0, 0, 0, 0] and flagged["crop_status"].tolist() == [0, 0, 2, 0]
    keep = [0, 1, 3]
    for k in ("euler", "joint_cam", "axis_angle", "reba", "rula", "status"):
        assert np.array_equal(usual[k][keep], flagged[k][keep], equal_nan=True), k
    # row 2 is the result of an all-zero crop, not of the good box
    blank = pipe(torch.zeros((B, 3, 224, 224), device=gpu_device))
    FramePipeline.wait(blank)
    assert np.array_equal(flagged["joint_cam"][2], blank["joint_cam"][0].cpu().numpy())
    assert not np.array_equal(flagged["joint_cam"][2], usual["joint_cam"][2])
