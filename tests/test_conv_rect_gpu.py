"""Every stand-alone convolution entry on rectangular maps (H != W; tests/conv_rect_cases.py has the cases and why), through
ops.* with out=, every tensor inside a guard-band arena (tests/guard_band.py) and once more on plain tensors, the same bits: a
read beside a rectangular tensor shows as a NaN, a store beside it as a touched guard.

Criteria are the entries' own (conv_rect_cases.check): fp32 against fp64 within 2e-5 max(1, max |ref|); one bf16 convolution
within |ref| 2^-8 + 2e-3; the bf16 conv2 + conv3 within |ref| 2^-7 + 2e-2 of its emulation -- and the bit relations the suite
claims on square maps: cfg 8 == cfg 7, the row panel (100) == cfg 8, every unit shape of the register-weights kernel (400) ==
T = 2 / NB = 1, cfgs 300 / 301 / 302 == cfg 13, conv2 + conv3 in one kernel == two launches on cfg 8, the dual-source forms 100 /
300 / 301 == the tile kernel's dual K loop.  tests/test_conv_rect_checker.py proves on the CPU that these criteria reject every
index defect that a square map hides.  Each family's worst max |gpu - fp64| / scale is reported through conftest.measured, beside the
square maps' parity maxima."""
import pytest
import torch

import conv_rect_cases as rc
import guard_band as gb
from conftest import measured
from poserisk_release_amd import _lib, ops

pytestmark = pytest.mark.gpu

_WORST = {}


def _cases(*families):
    cs = [c for f in families for c in rc.of_family(f)]
    return pytest.mark.parametrize("c", cs, ids=[c.name for c in cs])


def _dtype(c):
    return torch.bfloat16 if rc.FAMILIES[c.family].bf16 else torch.float32


def _precision(c):
    return "bf16" if rc.FAMILIES[c.family].bf16 else "fp32"


def _checked(c, with_res, y, what):
    """The family's criterion, and its worst scaled error so far into the parity maxima."""
    err = rc.scaled_error(c, with_res, y.float())
    _WORST[c.family] = max(_WORST.get(c.family, 0.0), err)
    measured(f"conv_rect {c.family} max |gpu - fp64| / max(1, max |fp64|)", _WORST[c.family], None if rc.FAMILIES[c.family].bf16 else 2e-5)
    rc.check(c, with_res, y, what)
    return y


def _guarded(call, inputs, out_shape, dt):
    """call(ins, out) -> y: once with every tensor in an arena (out: the arena's view), once on plain tensors (out None): the
    same bits."""
    got = gb.run_guarded(lambda i, o: call(i, o["y"]), inputs, {"y": (out_shape, dt)})["y"]
    plain = call({k: v.clone() for k, v in inputs.items()}, None)
    assert plain.dtype == got.dtype and torch.equal(plain, got), "placement changed the result"
    return got


def _conv_inputs(c, dev, with_res):
    d = rc.data(c)
    ins = {"x": d["x"].to(dev, _dtype(c))}
    if with_res:
        ins["res"] = d["res"].to(dev, _dtype(c))
    return ins


def _conv_call(c, cfg):
    d = rc.data(c)
    w, bias = d["w"].numpy(), d["bias"]

    def call(i, out, cfg=cfg):
        return ops.conv2d_nhwc(i["x"], w, bias, i.get("res"), stride=c.stride, pad=c.pad, relu=True, tile_cfg=cfg,
                               precision=_precision(c), out=out)[0]
    return call


def _conv(c, dev, cfg, with_res):
    """pr_conv2d_nhwc on the case with tile_cfg `cfg`, guarded, held against the family's criterion -> (y, call, inputs)."""
    Ho, Wo = rc.out_extent(c)
    ins, call = _conv_inputs(c, dev, with_res), _conv_call(c, cfg)
    y = _checked(c, with_res, _guarded(call, ins, (c.B, Ho, Wo, c.cout), _dtype(c)), (c.name, cfg, with_res))
    return y, call, ins


@_cases("tile_f32")
def test_tile_kernel_f32(gpu_device, c):
    """The fp32 LDS-DMA tile kernel: the heuristic's choice, the 128x64 tile and the 64x64 tile (whole tiles and the quarter
    tail), whose bits are the same."""
    for with_res in rc.FAMILIES[c.family].residual:
        y = {cfg: _conv(c, gpu_device, cfg, with_res)[0] for cfg in rc.FAMILIES[c.family].cfgs}
        assert torch.equal(y[8], y[7]), (c.name, with_res, int((y[8] != y[7]).sum()))


@_cases("splitk")
def test_split_k(gpu_device, c):
    for with_res in rc.FAMILIES[c.family].residual:
        for cfg in rc.FAMILIES[c.family].cfgs:
            _conv(c, gpu_device, cfg, with_res)


@_cases("panel")
def test_row_panel_has_the_tile_kernels_bits(gpu_device, c):
    for with_res in rc.FAMILIES[c.family].residual:
        y, call, ins = _conv(c, gpu_device, 100, with_res)
        assert torch.equal(y, call(ins, None, cfg=8))


@_cases("regw")
def test_register_weights_unit_shapes_have_the_same_bits(gpu_device, c, monkeypatch):
    """As test_conv_register_weights_unit_shapes_have_the_same_bits relates them: every (T, NB), and the defaults, give the bits
    of T = 2, NB = 1."""
    for with_res in rc.FAMILIES[c.family].residual:
        monkeypatch.delenv("POSERISK_REGW_T", raising=False)
        monkeypatch.delenv("POSERISK_REGW_NB", raising=False)
        y, call, ins = _conv(c, gpu_device, 400, with_res)
        monkeypatch.setenv("POSERISK_REGW_T", "2")
        monkeypatch.setenv("POSERISK_REGW_NB", "1")
        want = call(ins, None).clone()
        assert torch.equal(y, want)
        for T in (1, 2):
            for NB in (1, 2, 4):
                monkeypatch.setenv("POSERISK_REGW_T", str(T))
                monkeypatch.setenv("POSERISK_REGW_NB", str(NB))
                assert torch.equal(call(ins, None), want), (T, NB)


@_cases("wino")
def test_winograd(gpu_device, c):
    """F(2x2,3x3) and F(4x4,3x3) on both point sets: th != tw in every case; also within 2e-5 * scale of the direct kernel."""
    ref = rc.reference(c, False)
    scale = max(1.0, float(ref.abs().max()))
    direct = _conv_call(c, 8)(_conv_inputs(c, gpu_device, False), None)
    for cfg in rc.FAMILIES[c.family].cfgs:
        y, _, _ = _conv(c, gpu_device, cfg, False)
        assert float((y - direct).abs().max()) < 2e-5 * scale, cfg


@_cases("tile_bf16")
def test_tile_kernel_bf16(gpu_device, c):
    """Every tile configuration that accepts the shape, as test_conv_bf16_matches_emulation runs them."""
    ran = 0
    for cfg in range(6, _lib.load().pr_conv_num_tile_cfgs()):
        try:
            _conv(c, gpu_device, cfg, True)
        except _lib.PoseRiskHipError as e:
            assert "not a multiple of tile N" in str(e) or "bad channels" in str(e) or (cfg == 18 and "retired" in str(e)), str(e)
            continue
        ran += 1
    assert ran >= 1


@_cases("expand", "bal")
def test_persistent_bf16_kernels_have_the_tile_kernels_bits(gpu_device, c):
    """300 (weights in registers, + bias + residual), 301 / 302 (evenly dealt, no residual) == cfg 13."""
    (with_res,) = rc.FAMILIES[c.family].residual
    for cfg in rc.FAMILIES[c.family].cfgs:
        y, call, ins = _conv(c, gpu_device, cfg, with_res)
        assert torch.equal(y, call(ins, None, cfg=13)), cfg


@_cases("dual_f32", "dual_bf16")
def test_dual_source(gpu_device, c):
    """pr_conv1x1_dual_nhwc at stride2 = 2 with H2 = 2 Ho - 1 beside W2 = 2 Wo and the reverse; the row panel (100), the
    register-resident weights (300) and the evenly dealt kernel (301) have the bits of the tile kernel's dual K loop."""
    d, dt = rc.data(c), _dtype(c)
    w1, w2 = d["w"][:, :, 0, 0].numpy(), d["w2"].numpy()
    ins = {"t": d["x"].to(gpu_device, dt), "x": d["x2"].to(gpu_device, dt)}

    def call(i, out, cfg):
        return ops.conv1x1_dual_nhwc(i["t"], w1, i["x"], w2, d["bias"], stride2=2, relu=True, tile_cfg=cfg, precision=_precision(c), out=out)

    base = None
    for cfg in rc.FAMILIES[c.family].cfgs:
        y = _guarded(lambda i, o, cfg=cfg: call(i, o, cfg), ins, (c.B, c.H, c.W, c.cout), dt)
        _checked(c, False, y, (c.name, cfg))
        if cfg in (8, 13):
            base = y
        elif cfg >= 100:
            assert torch.equal(y, base), cfg


@_cases("fused_f32", "fused_bf16")
def test_conv3x3_conv1x1(gpu_device, c):
    """conv2 + conv3 of a layer1 Bottleneck in one kernel, with and without the residual; the bits of the two separate launches on
    the 64x64 tile."""
    d, dt, precision = rc.data(c), _dtype(c), _precision(c)
    w2, w3 = d["w"].numpy(), d["w3"].numpy()
    for with_res in rc.FAMILIES[c.family].residual:
        ins = {"x": d["x"].to(gpu_device, dt)}
        if with_res:
            ins["res"] = d["res3"].to(gpu_device, dt)

        def call(i, out):
            return ops.conv3x3_conv1x1_nhwc(i["x"], w2, d["bias"], w3, d["bias3"], i.get("res"), relu=True, precision=precision, out=out)

        y = _checked(c, with_res, _guarded(call, ins, (c.B, c.H, c.W, c.n3), dt), (c.name, with_res))
        t2, _ = ops.conv2d_nhwc(ins["x"], w2, d["bias"], None, stride=1, pad=1, relu=True, tile_cfg=8, precision=precision)
        y2, _ = ops.conv2d_nhwc(t2, w3.reshape(c.n3, 64, 1, 1), d["bias3"], ins.get("res"), relu=True, tile_cfg=8, precision=precision)
        assert torch.equal(y, y2)


def test_refusals_on_a_rectangle(gpu_device):
    """What the entries refuse by name they refuse on a rectangle too: the Winograd forms at stride 2, a kernel that is not square."""
    c = rc.BY_NAME["wino-2x5x11-64to192-k3s1"]
    d = rc.data(c)
    x = d["x"].to(gpu_device)
    for cfg in rc.FAMILIES["wino"].cfgs:
        with pytest.raises(_lib.PoseRiskHipError, match="Winograd"):
            ops.conv2d_nhwc(x, d["w"].numpy(), d["bias"], None, stride=2, pad=1, relu=True, tile_cfg=cfg)
    for precision in ("fp32", "bf16"):
        with pytest.raises(_lib.PoseRiskHipError, match="square kernels only"):
            ops.conv2d_nhwc(x, d["w"].numpy()[:, :, :1, :], d["bias"], None, stride=1, pad=0, relu=True, tile_cfg=8, precision=precision)
