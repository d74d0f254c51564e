"""layer1's 3x3 convolutions (64 -> 64 channels at 56x56) as Winograd F(4x4,3x3) in ONE launch (csrc/conv_wino64.hip): the
kernel through its stand-alone entry (pr_conv3x3_wino64_nhwc) against an fp64 im2col reference, alone (layer1.0's conv2)
and with conv3 + residual + ReLU behind it (layer1.1 / layer1.2, against conv3x3_conv1x1_f32 too), and the handle's routing
(POSERISK_WINO_LAYER1 = 0 | 1 | 2, read once per handle: none, layer1.0's conv2, all three).

Maps that 4x4 tiles do not cover exactly (8x12 is covered; 13x6 is not, 4x4 is a single tile in a 16-tile unit) WORK: the
tiles that overhang the map read zeros and their outputs are dropped by the buffer range check.  Tolerance: the criterion of
test_conv_winograd_matches_torch_and_direct for the three-launch form, 2e-5 of the layer's scale max(1, max |ref|)."""
import numpy as np
import pytest
import torch

from conftest import measured
from kernel_refs import wino64_layer as _layer, wino64_ref64 as _ref64
from poserisk_release_amd import _lib, ops, synth
from poserisk_release_amd.hmr import HMR

pytestmark = pytest.mark.gpu

SHAPES = [(2, 56, 56), (3, 8, 12), (1, 4, 4), (2, 13, 6)]      # (frames, H, W)
TOL = 2e-5


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


@pytest.mark.parametrize("form", [5, 4])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_wino64_conv2_matches_fp64(gpu_device, shape, form):
    x, w2, b2, _, _, _ = _layer(shape)
    ref = _ref64(x, w2, b2)
    y = ops.conv3x3_wino64_nhwc(_t(x, gpu_device), w2, b2, form=form).cpu().numpy()
    scale = max(1.0, np.abs(ref).max())
    err = np.abs(y - ref).max()
    measured(f"wino64 conv2 form {form} {shape}: max |gpu - fp64| / scale", err / scale, TOL)
    assert err < TOL * scale


@pytest.mark.parametrize("form", [5, 4])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_wino64_conv2_conv3_matches_fp64_and_the_direct_kernel(gpu_device, shape, form):
    x, w2, b2, w3, b3, res = _layer(shape)
    ref = _ref64(x, w2, b2, w3, b3, res)
    y = ops.conv3x3_wino64_nhwc(_t(x, gpu_device), w2, b2, w3, b3, _t(res, gpu_device), form=form)
    yd = ops.conv3x3_conv1x1_nhwc(_t(x, gpu_device), w2, b2, w3, b3, _t(res, gpu_device))
    scale = max(1.0, np.abs(ref).max())
    err = np.abs(y.cpu().numpy() - ref).max()
    errd = float((y - yd).abs().max())
    measured(f"wino64 conv2+conv3 form {form} {shape}: max |gpu - fp64| / scale", err / scale, TOL)
    measured(f"wino64 conv2+conv3 form {form} {shape}: max |gpu - conv3x3_conv1x1_f32| / scale", errd / scale, TOL)
    assert err < TOL * scale
    assert errd < TOL * scale
    # without a residual, and a narrower conv3
    y0 = ops.conv3x3_wino64_nhwc(_t(x, gpu_device), w2, b2, w3[:64], b3[:64], None, form=form).cpu().numpy()
    ref0 = _ref64(x, w2, b2, w3[:64], b3[:64], np.zeros_like(res[..., :64]))
    assert np.abs(y0 - ref0).max() < TOL * max(1.0, np.abs(ref0).max())


def test_wino64_refuses_other_shapes_by_name(gpu_device):
    x = torch.zeros((1, 8, 8, 128), device=gpu_device)
    w = np.zeros((128, 128, 3, 3), np.float32)
    with pytest.raises(_lib.PoseRiskHipError, match="Cin = Cout = 64"):
        ops.conv3x3_wino64_nhwc(x, w, np.zeros(128, np.float32))
    x = torch.zeros((1, 8, 8, 64), device=gpu_device)
    w = np.zeros((64, 64, 3, 3), np.float32)
    with pytest.raises(_lib.PoseRiskHipError, match="form"):
        ops.conv3x3_wino64_nhwc(x, w, np.zeros(64, np.float32), form=2)
    with pytest.raises(_lib.PoseRiskHipError, match="N3"):
        ops.conv3x3_wino64_nhwc(x, w, np.zeros(64, np.float32), np.zeros((96, 64), np.float32), np.zeros(96, np.float32))


@pytest.mark.parametrize("fused", [False, True], ids=["conv2", "conv2_conv3"])
def test_wino64_frame_bits_do_not_depend_on_the_batch(gpu_device, fused):
    """A frame alone, inside a batch of 64 (at any place in it), and run twice: the same bits."""
    x, w2, b2, w3, b3, res = _layer((64, 56, 56))
    xg, rg = _t(x, gpu_device), _t(res, gpu_device)

    def run(lo, hi):
        if fused:
            return ops.conv3x3_wino64_nhwc(xg[lo:hi], w2, b2, w3, b3, rg[lo:hi])
        return ops.conv3x3_wino64_nhwc(xg[lo:hi], w2, b2)

    full = run(0, 64)
    assert torch.equal(full, run(0, 64))
    for i in (0, 37, 63):
        assert torch.equal(run(i, i + 1)[0], full[i])
    assert torch.equal(run(5, 12), full[5:12])


def _handle(monkeypatch, gpu_device, sd, switch, **kw):
    if switch is None:
        monkeypatch.delenv("POSERISK_WINO_LAYER1", raising=False)
    else:
        monkeypatch.setenv("POSERISK_WINO_LAYER1", switch)
    m = HMR(max_batch=64, **kw).to(gpu_device)
    m.load_state_dict(sd)
    counts = m.plan_counts(64)      # creates the handle: the switch is read here, once
    return m, counts


def test_handle_routes_layer1_by_the_switch(gpu_device, monkeypatch):
    sd = synth.hmr_state_dict(seed=1)
    x = _t(synth.crops(4, seed=2), gpu_device)
    outs = {}
    for key, switch, kw in [("unset", None, {}), ("on", "1", {}), ("all", "2", {}), ("off", "0", {}), ("direct_on", "1", dict(conv_form="direct")),
                            ("direct_off", "0", dict(conv_form="direct")), ("w4_on", "1", dict(conv_form="winograd4")),
                            ("w244_on", "1", dict(conv_form="winograd244")), ("w244_off", "0", dict(conv_form="winograd244"))]:
        m, counts = _handle(monkeypatch, gpu_device, sd, switch, **kw)
        assert counts == (47, 0 if "direct" in key else 10), (key, counts)
        outs[key] = [m.encode_until(x, 3).clone()] + [t.clone() for t in m(x, return_features=True)]
    # the shipped default (variable unset) is value 1: layer1.0's conv2 routed
    for a, b in zip(outs["unset"], outs["on"]):
        assert torch.equal(a, b)
    # the default form: the route really changed, within the fp32 tolerance
    blk_on, blk_off = outs["on"][0], outs["off"][0]
    assert not torch.equal(blk_on, blk_off)
    scale = max(1.0, float(blk_off.abs().max()))
    measured("layer1 output, switch on vs off: max |diff| / scale", float((blk_on - blk_off).abs().max()) / scale, 1e-4)
    assert float((blk_on - blk_off).abs().max()) < 1e-4 * scale
    for a, b in zip(outs["on"][1:4], outs["off"][1:4]):      # rotation matrices, betas, camera
        assert float((a - b).abs().max()) < 1e-4
    # 2 = layer1.1's and layer1.2's conv2 + conv3 launches as well: another route again, within the same tolerance
    blk_all = outs["all"][0]
    assert not torch.equal(blk_all, blk_on) and not torch.equal(blk_all, blk_off)
    measured("layer1 output, switch 2 vs off: max |diff| / scale", float((blk_all - blk_off).abs().max()) / scale, 1e-4)
    assert float((blk_all - blk_off).abs().max()) < 1e-4 * scale
    # "direct" and a handle whose layer2 runs F(2x2) keep today's kernels for layer1: bit-equal either way
    for a, b in zip(outs["direct_on"], outs["direct_off"]):
        assert torch.equal(a, b)
    for a, b in zip(outs["w244_on"], outs["w244_off"]):
        assert torch.equal(a, b)
    # form 4 covers layer1 on its own points
    assert not torch.equal(outs["w4_on"][0], blk_on) and not torch.equal(outs["w4_on"][0], blk_off)
