"""Every stand-alone kernel entry with all of its tensors inside guard-band arenas (tests/guard_band.py): inputs between NaN
(255, 0x7fffffff) guards, outputs between canary guards, at the smallest shapes where the kernel's indexing still has every
edge -- a first and a last frame, a ragged last tile (M no multiple of 16), fewer rows than one fragment, a single pixel.

Why: the hot kernels address through raw buffer descriptors whose range check covers the vector offset only; wave-uniform
terms ride in the scalar offset, which the hardware does not check, so a halo lane of the first frame's first row or the
last frame's last row, a row >= M of a ragged tile, or the stride-2 second source's last pixel must be routed out of range
by hand.  A mistake that reaches into a neighbouring frame fails the parity tests; one that reaches OUTSIDE the tensor does
not, because torch's caching allocator puts slack or a dead tensor there.  Here it lands in a guard.

Each guarded call is checked three ways: the guards came back intact and the outputs hold neither NaN nor canary
(run_guarded); the outputs equal, bit for bit, the same call on plain tensors (placement must not change arithmetic); and
they meet the reference and tolerance of the entry's own parity test (tests/kernel_refs.py holds what both share).

Out of this fence's reach: the handles' internal workspaces (hipMalloc'ed inside the library; the internal fence of
tests/test_internal_fence_gpu.py covers them), and reads outside a tensor whose value never reaches an output
(guard_band.py's docstring)."""
import numpy as np
import pytest
import torch

import encoder_ref as er
import guard_band as gb
import kernel_refs as kr
from conftest import golden
from oracle import coord_ref, crop_ref, hmr_ref, pipeline_ref, reba_ref, rula_ref, smpl_ref
from poserisk_release_amd import ops, synth
from poserisk_release_amd.hmr import HMR
from poserisk_release_amd.pipeline import FramePipeline
from poserisk_release_amd.smpl_layer import SMPLLayer

pytestmark = pytest.mark.gpu

TOL_F32 = 1e-4   # tests/test_hip_parity.py's tolerances of the whole model: SMPL pose / shape / camera ...
TOL_MM = 0.10    # ... and joint_cam in millimetres
F32, BF16, F64, I32 = torch.float32, torch.bfloat16, torch.float64, torch.int32


def _o(outs, name):
    return None if outs is None else outs[name]


def guarded(call, inputs, outputs, skip_plain=(), **kw):
    """call(ins, outs) -> {name: tensor} runs the entry on the tensors of `ins`, writing into `outs` (None: fresh outputs).
    Once inside arenas (guard_band.run_guarded), once on plain tensors: the same bits."""
    got = gb.run_guarded(lambda i, o: call(i, o), inputs, outputs, **kw)
    plain = call({k: v.clone() for k, v in inputs.items()}, None)
    for name, t in got.items():
        if name not in skip_plain:
            assert plain[name].dtype == t.dtype and torch.equal(plain[name], t), f"{name}: placement changed the result"
    return got


def test_the_fence_sees_a_one_element_overrun_on_the_gpu(gpu_device):
    """The harness' own check on device memory (tests/test_guard_band_cpu.py has the rest on the CPU): a "kernel" that
    stores one element behind its output, one that reads one element past its input."""
    x = torch.arange(1.0, 61.0, device=gpu_device).reshape(3, 5, 4)
    past = lambda t, k: t.as_strided((1,), (1,), t.storage_offset() + t.numel() + k)

    def stores_behind(i, o):
        torch.mul(i["x"], 2.0, out=o["y"])
        past(o["y"], 0).fill_(1.0)

    def reads_past(i, o):
        torch.mul(i["x"], 2.0, out=o["y"])
        o["y"].view(-1)[-1:] += 0.0 * past(i["x"], 0)

    with pytest.raises(AssertionError, match=r"output y .*BEHIND the tensor touched: 1 elements, first at \+0"):
        gb.run_guarded(stores_behind, {"x": x}, {"y": ((3, 5, 4), F32)})
    with pytest.raises(AssertionError, match="output y: 1 NaN, first at flat element 59"):
        gb.run_guarded(reads_past, {"x": x}, {"y": ((3, 5, 4), F32)})
    y = gb.run_guarded(lambda i, o: torch.mul(i["x"], 2.0, out=o["y"]), {"x": x}, {"y": ((3, 5, 4), F32)})["y"]
    assert torch.equal(y, x * 2) and y.data_ptr() % 256 == 0


def _rng(*key):
    return np.random.default_rng(abs(hash(key)) % 2 ** 32)


def _ids(c):
    return "x".join(str(v) for v in c) if isinstance(c, tuple) else str(c)


# ------------------------------------------------------------------------------------------------
# ops.conv2d_nhwc
# ------------------------------------------------------------------------------------------------
_CONV_DATA = {}


def _conv_data(shape, bf):
    """Seeded input, weights, bias, residual of a conv shape (B, H, Cin_real, Cin, Cout, k, stride, pad) and its fp64
    references without / with the residual (+ ReLU): built once per shape, shared by the tile configurations."""
    if (shape, bf) not in _CONV_DATA:
        B, H, Cr, Cin, Cout, k, s, p = shape
        rng = _rng(*shape)
        rnd = kr.bf16_round if bf else (lambda t: t)
        x = rnd(torch.from_numpy(rng.standard_normal((B, H, H, Cin)).astype(np.float32)))
        x[..., Cr:] = 0
        w = rnd(torch.from_numpy((rng.standard_normal((Cout, Cr, k, k)) / np.sqrt(Cr * k * k)).astype(np.float32))).numpy()
        bias = rng.standard_normal(Cout).astype(np.float32)
        Ho = (H + 2 * p - k) // s + 1
        res = rnd(torch.from_numpy(rng.standard_normal((B, Ho, Ho, Cout)).astype(np.float32)))
        refs = {r: kr.conv_ref64(x, w, bias, res if r else None, stride=s, pad=p, relu=True) for r in (False, True)}
        _CONV_DATA[(shape, bf)] = (x, w, bias, res, refs, Ho)
    return _CONV_DATA[(shape, bf)]


def _run_conv(dev, cfg, shape, with_res, bf):
    B, H, Cr, Cin, Cout, k, s, p = shape
    x, w, bias, res, refs, Ho = _conv_data(shape, bf)
    dt = BF16 if bf else F32
    ins = {"x": x.to(dev, dt)}
    if with_res:
        ins["res"] = res.to(dev, dt)

    def call(i, o, cfg=cfg):
        y, _ = ops.conv2d_nhwc(i["x"], w, bias, i.get("res"), stride=s, pad=p, relu=True, tile_cfg=cfg,
                               precision="bf16" if bf else "fp32", out=_o(o, "y"))
        return {"y": y}

    y = guarded(call, ins, {"y": ((B, Ho, Ho, Cout), dt)})["y"]
    (kr.assert_close_bf16 if bf else kr.assert_close_f32)(y, refs[with_res], (cfg, shape, with_res))
    return y, call, ins


def _f32_conv_cases():
    tile = [(1, 9, 64, 64, 64, 3, 1, 1), (2, 5, 64, 64, 128, 3, 2, 1), (1, 5, 96, 96, 64, 1, 1, 0),
            (2, 30, 3, 4, 64, 7, 2, 3)]                                     # the 7x7 / 2 / pad 3 stem, 3 real channels of 4
    cases = [(c, t) for c in (-1, 7, 8) for t in tile]
    cases += [(c, t) for c in (202, 203, 204) for t in [(2, 9, 64, 64, 128, 3, 1, 1), (1, 5, 96, 96, 64, 1, 1, 0)]]    # split-K
    cases += [(100, t) for t in [(1, 5, 128, 128, 256, 1, 1, 0), (1, 3, 128, 128, 256, 1, 1, 0)]]                       # row panel
    cases += [(400, t) for t in [(1, 5, 128, 128, 256, 1, 1, 0), (3, 7, 256, 256, 192, 1, 1, 0)]]                       # register weights
    cases = [(c, t, r) for c, t in cases for r in (False, True)]
    # Winograd F(2x2), F(4x4) on both point sets: the entry takes no residual
    cases += [(c, t, False) for c in (-2, -4, -5) for t in [(2, 9, 64, 64, 192, 3, 1, 1), (1, 7, 512, 512, 512, 3, 1, 1)]]
    return cases


@pytest.mark.parametrize("cfg,shape,with_res", _f32_conv_cases(), ids=_ids)
def test_conv_f32(gpu_device, cfg, shape, with_res):
    _run_conv(gpu_device, cfg, shape, with_res, bf=False)


def _bf16_conv_cases():
    # tests/test_hip_parity.py's BF16_CONV_CASES: its two smallest on the 128x64 tile (13), its smallest with >= 256 output
    # pixels on the 256x64 tile (11)
    cases = [(13, (1, 9, 64, 64, 64, 3, 1, 1), r) for r in (False, True)]
    cases += [(13, (3, 7, 512, 512, 512, 3, 1, 1), r) for r in (False, True)]
    cases += [(11, (2, 28, 128, 128, 128, 3, 1, 1), r) for r in (False, True)]
    # register-resident weights (300): 1x1 expansion + bias + residual
    cases += [(300, (B, H, K, K, N, 1, 1, 0), True) for B, H in ((1, 9), (3, 5), (1, 1)) for K, N in ((128, 512), (256, 1024))]
    # evenly dealt persistent kernel (301 / 302): no residual
    cases += [(c, (B, H, Cin, Cin, Cout, k, s, k // 2), False) for B, H, Cin, Cout, k, s, c in
              [(1, 9, 64, 128, 1, 1, 301), (7, 5, 128, 256, 1, 1, 302), (1, 1, 64, 128, 3, 1, 301), (7, 5, 192, 256, 3, 1, 301),
               (2, 28, 256, 256, 3, 2, 301)]]
    return cases


@pytest.mark.parametrize("cfg,shape,with_res", _bf16_conv_cases(), ids=_ids)
def test_conv_bf16(gpu_device, cfg, shape, with_res):
    y, call, ins = _run_conv(gpu_device, cfg, shape, with_res, bf=True)
    if cfg >= 300:      # these kernels' own tests: the tile kernel's bits
        assert torch.equal(y, call(ins, None, cfg=13)["y"])


# ------------------------------------------------------------------------------------------------
# ops.conv1x1_dual_nhwc: the second source is 2 Ho - 1 wide for odd Ho, so the stride-2 read of the last output pixel is
# the second source's last pixel
# ------------------------------------------------------------------------------------------------
def _dual_cases():
    cases = [("fp32", c, (1, 5, 64, 128, 64)) for c in (-1, 8, 100)]
    cases += [("bf16", c, (B, Ho, 128, 256, 512)) for c in (13, 300) for B, Ho in ((1, 5), (3, 9), (1, 1))]
    cases += [("bf16", 301, (2, 9, 128, 256, 512)), ("bf16", 301, (1, 1, 64, 64, 128))]
    return cases


@pytest.mark.parametrize("precision,cfg,shape", _dual_cases(), ids=_ids)
def test_conv1x1_dual(gpu_device, precision, cfg, shape):
    B, Ho, C1, C2, N = shape
    H2 = 2 * Ho - 1 if Ho % 2 else 2 * Ho
    bf = precision == "bf16"
    dt = BF16 if bf else F32
    rnd = kr.bf16_round if bf else (lambda t: t)
    rng = _rng(*shape)
    t = rnd(torch.from_numpy(rng.standard_normal((B, Ho, Ho, C1)).astype(np.float32)))
    x = rnd(torch.from_numpy(rng.standard_normal((B, H2, H2, C2)).astype(np.float32)))
    w1 = rnd(torch.from_numpy((rng.standard_normal((N, C1)) / np.sqrt(C1)).astype(np.float32))).numpy()
    w2 = rnd(torch.from_numpy((rng.standard_normal((N, C2)) / np.sqrt(C2)).astype(np.float32))).numpy()
    bias = rng.standard_normal(N).astype(np.float32)
    ref = kr.dual_ref64(t, w1, x, w2, bias, 2)

    def call(i, o, cfg=cfg):
        return {"y": ops.conv1x1_dual_nhwc(i["t"], w1, i["x"], w2, bias, stride2=2, relu=True, tile_cfg=cfg, precision=precision,
                                           out=_o(o, "y"))}

    ins = {"t": t.to(gpu_device, dt), "x": x.to(gpu_device, dt)}
    y = guarded(call, ins, {"y": ((B, Ho, Ho, N), dt)})["y"]
    (kr.assert_close_bf16 if bf else kr.assert_close_f32)(y, ref, (cfg, shape))
    if cfg >= 100:      # row panel / register weights / evenly dealt: the tile kernel's dual-source K loop, bit for bit
        assert torch.equal(y, call(ins, None, cfg=13 if bf else 8)["y"])


# ------------------------------------------------------------------------------------------------
# conv2 + conv3 of a layer1 Bottleneck in one kernel
# ------------------------------------------------------------------------------------------------
# (B, H, Cin, N3, residual).  bf16 refuses Cin = 32 by name ("Cin must be a power of two >= 64"): in its place the nearest
# shape of test_conv3x3_conv1x1_fused_bf16, (3, 14, 64 -> 128) without residual
@pytest.mark.parametrize("precision,case", [("fp32", (1, 5, 32, 64, True)), ("fp32", (1, 5, 32, 64, False)), ("fp32", (1, 9, 64, 256, True)),
                                            ("bf16", (3, 14, 64, 128, False)), ("bf16", (1, 9, 64, 256, True))], ids=_ids)
def test_conv3x3_conv1x1(gpu_device, precision, case):
    B, H, Cin, N3, with_res = case
    bf = precision == "bf16"
    dt = BF16 if bf else F32
    rnd = kr.bf16_round if bf else (lambda t: t)
    rng = _rng(*case)
    x = rnd(torch.from_numpy(rng.standard_normal((B, H, H, Cin)).astype(np.float32)))
    w2 = rnd(torch.from_numpy((rng.standard_normal((64, Cin, 3, 3)) / np.sqrt(Cin * 9)).astype(np.float32)))
    b2 = rng.standard_normal(64).astype(np.float32)
    w3 = rnd(torch.from_numpy((rng.standard_normal((N3, 64)) / 8).astype(np.float32)))
    b3 = rng.standard_normal(N3).astype(np.float32)
    res = rnd(torch.from_numpy(rng.standard_normal((B, H, H, N3)).astype(np.float32))) if with_res else None

    def call(i, o):
        return {"y": ops.conv3x3_conv1x1_nhwc(i["x"], w2.numpy(), b2, w3.numpy(), b3, i.get("res"), relu=True, precision=precision,
                                              out=_o(o, "y"))}

    ins = {"x": x.to(gpu_device, dt)}
    if with_res:
        ins["res"] = res.to(gpu_device, dt)
    y = guarded(call, ins, {"y": ((B, H, H, N3), dt)})["y"]
    if bf:      # test_conv3x3_conv1x1_fused_bf16's criterion: one flip of a t2 rounding on top of the output's own ulp
        ref = kr.fused_bf16_emulation(x, w2, b2, w3, b3, res)
        assert bool(((y.float().cpu() - ref).abs() <= ref.abs() * 2.0 ** -7 + 2e-2).all())
    else:
        kr.assert_close_f32(y, kr.fused_ref64(x, w2, b2, w3, b3, res), case)
    # ... and the bits of the two separate launches on the 64x64 tile
    t2, _ = ops.conv2d_nhwc(ins["x"], w2.numpy(), b2, None, stride=1, pad=1, relu=True, tile_cfg=8, precision=precision)
    y2, _ = ops.conv2d_nhwc(t2, w3.numpy().reshape(N3, 64, 1, 1), b3, ins.get("res"), relu=True, tile_cfg=8, precision=precision)
    assert torch.equal(y, y2)


@pytest.mark.parametrize("fused", [False, True], ids=["conv2", "conv2_conv3"])
@pytest.mark.parametrize("form", [4, 5])
@pytest.mark.parametrize("shape", [(1, 9, 9), (2, 5, 5)], ids=_ids)
def test_conv3x3_wino64(gpu_device, shape, form, fused):
    B, H, W = shape
    x, w2, b2, w3, b3, res = kr.wino64_layer(shape)
    ins = {"x": torch.from_numpy(x).to(gpu_device)}
    if fused:
        ins["res"] = torch.from_numpy(res).to(gpu_device)

    def call(i, o):
        if fused:
            return {"y": ops.conv3x3_wino64_nhwc(i["x"], w2, b2, w3, b3, i["res"], form=form, out=_o(o, "y"))}
        return {"y": ops.conv3x3_wino64_nhwc(i["x"], w2, b2, form=form, out=_o(o, "y"))}

    y = guarded(call, ins, {"y": ((B, H, W, 256 if fused else 64), F32)})["y"]
    ref = kr.wino64_ref64(x, w2, b2, w3, b3, res) if fused else kr.wino64_ref64(x, w2, b2)
    assert np.abs(y.cpu().numpy() - ref).max() < 2e-5 * max(1.0, np.abs(ref).max())


# ------------------------------------------------------------------------------------------------
# whole Bottlenecks and stems in one kernel (bf16 blocks: rewritten onto the shared device vocabulary)
# ------------------------------------------------------------------------------------------------
def _run_bottleneck(dev, mid, case, first=False):
    B, H, W = case
    x, w1, w2, w3, wd, b = kr.bottleneck_inputs(mid, case, first)
    cout = w3.shape[0]
    fn = {64: ops.bottleneck_nhwc, 128: ops.bottleneck128_nhwc, 256: ops.bottleneck256_nhwc}[mid]
    extra = dict(wd=wd.numpy(), bd=b[3]) if first else {}

    def call(i, o):
        return {"y": fn(i["x"], w1.numpy(), b[0], w2.numpy(), b[1], w3.numpy(), b[2], out=_o(o, "y"), **extra)[0]}

    ins = {"x": x.to(dev, BF16)}
    y = guarded(call, ins, {"y": ((B, H, W, cout), BF16)})["y"]
    ref = kr.bottleneck_emulation(x, w1, b[0], w2, b[1], w3, b[2], wd, b[3] if first else None)
    slack = 3e-2 if mid == 64 else 5e-2           # the whole-block tests' criteria
    assert bool(((y.float().cpu() - ref).abs() <= ref.abs() * 2.0 ** -7 + slack).all())
    return y, ins["x"], (w1, w2, w3, wd, b)


@pytest.mark.parametrize("case", [(1, 9, 9), (2, 13, 6), (7, 1, 1)], ids=_ids)
@pytest.mark.parametrize("first", [False, True], ids=["plain", "first"])
def test_bottleneck64(gpu_device, case, first):
    y, xd, (w1, w2, w3, wd, b) = _run_bottleneck(gpu_device, 64, case, first)
    # the separate launches the kernel replaces: the same bits
    t1, _ = ops.conv2d_nhwc(xd, w1.numpy().reshape(64, -1, 1, 1), b[0], None, relu=True, tile_cfg=8, precision="bf16")
    if first:
        t2, _ = ops.conv2d_nhwc(t1, w2.numpy(), b[1], None, stride=1, pad=1, relu=True, tile_cfg=8, precision="bf16")
        b3d = (b[2].astype(np.float64) + b[3].astype(np.float64)).astype(np.float32)
        y2 = ops.conv1x1_dual_nhwc(t2, w3.numpy(), xd, wd.numpy(), b3d, relu=True, tile_cfg=8, precision="bf16")
    else:
        y2 = ops.conv3x3_conv1x1_nhwc(t1, w2.numpy(), b[1], w3.numpy(), b[2], xd, relu=True, precision="bf16")
    assert torch.equal(y, y2)


@pytest.mark.parametrize("mid,case", [(128, c) for c in [(1, 9, 9), (2, 13, 6), (1, 3, 31), (7, 1, 1)]] +
                         [(256, c) for c in [(1, 9, 9), (2, 13, 6), (1, 4, 8), (5, 1, 1)]], ids=_ids)
def test_bottleneck128_and_256(gpu_device, mid, case):
    y, xd, (w1, w2, w3, _, b) = _run_bottleneck(gpu_device, mid, case)
    t1, _ = ops.conv2d_nhwc(xd, w1.numpy().reshape(mid, 4 * mid, 1, 1), b[0], None, relu=True, tile_cfg=13, precision="bf16")
    t2, _ = ops.conv2d_nhwc(t1, w2.numpy(), b[1], None, pad=1, relu=True, tile_cfg=13, precision="bf16")
    y2, _ = ops.conv2d_nhwc(t2, w3.numpy().reshape(4 * mid, mid, 1, 1), b[2], xd, relu=True, tile_cfg=13, precision="bf16")
    assert torch.equal(y, y2)


@pytest.mark.parametrize("case", [(1, 30), (5, 2), (2, 58)], ids=_ids)
def test_stem_pool_bf16(gpu_device, case):
    B, H = case
    x, w, bias, ref = kr.stem_pool_bf16_case(case)

    def call(i, o):
        return {"y": ops.stem_pool_nhwc(i["x"], w.numpy(), bias, out=_o(o, "y"))[0]}

    y = guarded(call, {"x": x.to(gpu_device, BF16)}, {"y": ((B, H // 2, H // 2, 64), BF16)})["y"]
    got = y.float().cpu()
    assert not bool(((got - ref).abs() > ref.abs() * 2.0 ** -7 + 1e-6).any())
    assert float((got == ref).float().mean()) > 0.98


def test_stem_pool_f32(gpu_device):
    B = 2
    x, w, bias, ref, _ = kr.stem_pool_f32_case(B)

    def call(i, o):
        return {"y": ops.stem_pool_f32_nhwc(i["x"], w, bias, out=_o(o, "y"))[0]}

    y = guarded(call, {"x": torch.from_numpy(x).to(gpu_device)}, {"y": ((B, 56, 56, 64), F32)})["y"]
    assert np.abs(y.cpu().numpy() - ref).max() < 2e-5 * max(1.0, np.abs(ref).max())


TIMED_BLOCKS = {"bottleneck64": (64, False), "bottleneck64_first": (64, True), "bottleneck128": (128, False), "bottleneck256": (256, False)}


def _timed_entry(dev, entry):
    """-> call(repeats) of a stand-alone entry that takes `repeats`, on the smallest case of its test above."""
    if entry in TIMED_BLOCKS:
        mid, first = TIMED_BLOCKS[entry]
        x, w1, w2, w3, wd, b = kr.bottleneck_inputs(mid, (5, 1, 1) if mid == 256 else (7, 1, 1), first)
        fn = {64: ops.bottleneck_nhwc, 128: ops.bottleneck128_nhwc, 256: ops.bottleneck256_nhwc}[mid]
        extra = dict(wd=wd.numpy(), bd=b[3]) if first else {}
        xd = x.to(dev, BF16)
        return lambda repeats: fn(xd, w1.numpy(), b[0], w2.numpy(), b[1], w3.numpy(), b[2], repeats=repeats, **extra)
    if entry == "stem_pool_bf16":
        x, w, bias, _ = kr.stem_pool_bf16_case((5, 2))
        xd = x.to(dev, BF16)
        return lambda repeats: ops.stem_pool_nhwc(xd, w.numpy(), bias, repeats=repeats)
    x, w, bias, _, _ = kr.stem_pool_f32_case(2)
    xd = torch.from_numpy(x).to(dev)
    return lambda repeats: ops.stem_pool_f32_nhwc(xd, w, bias, repeats=repeats)


@pytest.mark.parametrize("entry", [*TIMED_BLOCKS, "stem_pool_bf16", "stem_pool_f32"])
def test_the_timed_loop_times_and_leaves_the_output_as_it_is(gpu_device, entry):
    """The event-timed `repeats` loop the stand-alone entries share: a time comes back, and the launches it adds write what the
    first one wrote."""
    call = _timed_entry(gpu_device, entry)
    y0, ms0 = call(0)
    y2, ms2 = call(2)
    assert ms0 is None and ms2 is not None and np.isfinite(ms2) and ms2 > 0
    assert torch.equal(y0, y2)


# ------------------------------------------------------------------------------------------------
# behind the encoder: rotations, Euler angles, scores
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 7])
def test_rot6d_to_rotmat(gpu_device, N):
    p = np.random.default_rng(1).standard_normal((N, 144)).astype(np.float32)
    ref = hmr_ref.rot6d_to_rotmat(torch.from_numpy(p)).view(N, 24, 3, 3).numpy()
    out = guarded(lambda i, o: {"r": ops.rot6d_to_rotmat(i["p"], out=_o(o, "r"))}, {"p": torch.from_numpy(p).to(gpu_device)},
                  {"r": ((N, 24, 3, 3), F32)})["r"]
    np.testing.assert_allclose(out.cpu().numpy(), ref, atol=2e-5)


# pose_to_euler_kernel: kEulerFramesPerBlock = 8 frames (x 24 joints = 192 threads) per workgroup
# (csrc/frame_kernels.hip), so 8 * 1 + 1 = 9 frames leave one frame in a second workgroup whose other seven
# frame slots -- and status slots -- must stay out of range
EULER_N = [1, 5, 8 * 1 + 1]


@pytest.mark.parametrize("N", EULER_N)
def test_pose_to_euler(gpu_device, N):
    g = golden("euler.npz")
    assert g["rotmat"].shape[0] >= N

    def call(i, o):
        out = None if o is None else (o["aa"], o["eul"], o["st"])
        aa, eul, st = ops.pose_to_euler(i["rot"], out=out)
        return {"aa": aa, "eul": eul, "st": st}

    got = guarded(call, {"rot": torch.from_numpy(g["rotmat"][:N].astype(np.float32)).to(gpu_device)},
                  {"aa": ((N, 24, 3), F32), "eul": ((N, 24, 3), F64), "st": ((N,), I32)})
    aa, eul = got["aa"].cpu().numpy(), got["eul"].cpu().numpy()
    np.testing.assert_allclose(aa, g["axis_angle"][:N], atol=1e-6)
    d, off, ulp, dg = kr.pose_to_euler_errors(aa, eul, g["axis_angle"][:N], g["euler_deg"][:N])
    assert d.max() < 1e-5 and (off <= ulp).all() and dg.max() < 2e-5
    assert got["st"].cpu().tolist() == [0] * N


@pytest.mark.parametrize("N", EULER_N)
def test_axis_angle_to_euler(gpu_device, N):
    """(No parity test of its own before this one: the Euler stage of test_pose_to_euler_matches_golden is its criterion --
    the oracle's axis_angle_to_euler_angle on the same float32 axis-angle, 1e-5 degrees.)"""
    aa = golden("euler.npz")["axis_angle"][:N].astype(np.float32)

    def call(i, o):
        eul, st = ops.axis_angle_to_euler(i["aa"], out=None if o is None else (o["eul"], o["st"]))
        return {"eul": eul, "st": st}

    got = guarded(call, {"aa": torch.from_numpy(aa).to(gpu_device)}, {"eul": ((N, 24, 3), F64), "st": ((N,), I32)})
    ref = np.stack([coord_ref.axis_angle_to_euler_angle(f) for f in aa])
    d = np.abs(got["eul"].cpu().numpy() - ref)
    assert np.minimum(d, 360 - d).max() < 1e-5
    assert got["st"].cpu().tolist() == [0] * N


# reba_kernel / rula_kernel: one frame per thread, 64 threads per workgroup: 64 + 1 frames
@pytest.mark.parametrize("N", [1, 64 + 1])
def test_reba_and_rula(gpu_device, N):
    pose = np.random.default_rng(11).uniform(-180, 180, (N, 24, 3))
    info = synth.EXAMPLE_INFO
    ins = {"pose": torch.from_numpy(pose).to(gpu_device)}
    reba = guarded(lambda i, o: {"s": ops.reba(i["pose"], info["REBA"], out=_o(o, "s"))}, ins, {"s": ((N, 10), I32)})["s"]
    rula = guarded(lambda i, o: {"s": ops.rula(i["pose"], info["RULA"], out=_o(o, "s"))}, ins, {"s": ((N, 12), I32)})["s"]
    np.testing.assert_array_equal(reba.cpu().numpy(), reba_ref.reba_packed(pose, info["REBA"]))
    np.testing.assert_array_equal(rula.cpu().numpy(), rula_ref.rula_packed(pose, info["RULA"]))


# ------------------------------------------------------------------------------------------------
# SMPL
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def smpl97():
    sm = synth.smpl_model(V=97, seed=2)
    return sm, smpl_ref.SMPLModel(**{k: sm[k] for k in ("v_template", "shapedirs", "posedirs", "J_regressor", "weights")})


# the handle's skinning kernel: register-tiled (max_batch <= 128, sparse weights), wave-split (the same, switched off), rows
SMPL_VARIANTS = {"skin_tile": (32, "1"), "skin_split_waves": (32, "0"), "skin_rows": (256, None)}


@pytest.mark.parametrize("B", [1, 5, 17])
@pytest.mark.parametrize("variant", list(SMPL_VARIANTS))
def test_smpl_forward_and_joint_cam(gpu_device, smpl97, monkeypatch, variant, B):
    sm, om = smpl97
    max_batch, tile = SMPL_VARIANTS[variant]
    if tile is None:
        monkeypatch.delenv("POSERISK_SMPL_TILE", raising=False)
    else:
        monkeypatch.setenv("POSERISK_SMPL_TILE", tile)          # read by pr_smpl_create
    layer = SMPLLayer(sm, device=gpu_device, max_batch=max_batch)
    layer._ensure()
    pose, betas = synth.poses(B, seed=40 + B), synth.betas(B, seed=41 + B)
    trans = (np.random.default_rng(B).standard_normal((B, 3)) * 0.2).astype(np.float32)

    def forward(i, o):
        v, j = layer(i["pose"], i["betas"], i["trans"], out=None if o is None else (o["verts"], o["joints"]))
        return {"verts": v, "joints": j}

    got = guarded(forward, {k: torch.from_numpy(a).to(gpu_device) for k, a in (("pose", pose), ("betas", betas), ("trans", trans))},
                  {"verts": ((B, 97, 3), F32), "joints": ((B, 24, 3), F32)})
    vr, jr = smpl_ref.smpl_forward(om, pose, betas, trans)
    np.testing.assert_allclose(got["verts"].cpu().numpy(), vr, atol=1e-5)
    np.testing.assert_allclose(got["joints"].cpu().numpy(), jr, atol=1e-5)

    def joint_cam(i, o):
        jc, v = layer.joint_cam(i["aa"], return_verts=True, out=None if o is None else (o["jc"], o["verts"]))
        return {"jc": jc, "verts": v}

    aa = pose.reshape(B, 24, 3).copy()
    ins = {"aa": torch.from_numpy(aa).to(gpu_device)}
    # joint_cam overwrites the root rows of its input in place (the reference's quirk): the one input a kernel may write
    got = guarded(joint_cam, ins, {"jc": ((B, 24, 3), F32), "verts": ((B, 97, 3), F32)}, mutated=("aa",))
    want = coord_ref.get_joint_cam(aa, lambda p, b: smpl_ref.smpl_forward(om, p, b))        # (overwrites aa's root rows too)
    np.testing.assert_allclose(got["jc"].cpu().numpy(), want, atol=1e-2)                    # millimetres
    assert np.all(aa[:, 0] == np.array([3.14, 0, 0], np.float32))
    # ... and no more of it than the root rows, not even on the plain tensor of the second run
    after = ins["aa"].clone()
    layer.joint_cam(after)
    np.testing.assert_array_equal(after.cpu().numpy(), aa)


# ------------------------------------------------------------------------------------------------
# crop front end
# ------------------------------------------------------------------------------------------------
def test_crop_frames(gpu_device):
    """Two frames of 37 x 53 between guards of 255 (the oracle's border is 0: a guard byte that takes part changes the crop).
    Boxes: over the first frame's top-left corner; over the last frame's bottom-right corner at 1:1 scale (output pixels land
    on the frame's last pixel pairs one by one: the pair that ends 1 byte before the end of the buffer takes the 8-byte
    load, the last pair -- whose 8 bytes would end 2 bytes past it -- must take the byte loads); wholly inside; wholly
    outside; and two frame indices out of range, which the kernel answers with a zero crop and status 1."""
    F, H, W = 2, 37, 53
    frames = np.random.default_rng(5).integers(1, 255, (F, H, W, 3), dtype=np.uint8)      # neither the border's 0 nor the guards' 255
    boxes = np.array([[1.5, 2.5, 30.0, 20.0], [W - 1.0, H - 1.0, 224 / 1.2, 224 / 1.2], [26.0, 18.0, 20.0, 14.0],
                      [-300.0, -300.0, 50.0, 50.0], [26.0, 18.0, 20.0, 14.0], [26.0, 18.0, 20.0, 14.0]], np.float32)
    idx = np.array([0, 1, 1, 0, 7, -2], np.int32)
    N = len(boxes)

    def call(i, o):
        crops, st = ops.crop_frames(i["frames"], i["boxes"], i["idx"], scale=1.2, return_status=True,
                                    out=None if o is None else (o["crops"], o["status"]))
        return {"crops": crops, "status": st}

    got = guarded(call, {"frames": torch.from_numpy(frames).to(gpu_device), "boxes": torch.from_numpy(boxes).to(gpu_device),
                         "idx": torch.from_numpy(idx).to(gpu_device)},
                  {"crops": ((N, 3, 224, 224), F32), "status": ((N,), I32)})
    crops = got["crops"].cpu().numpy()
    assert got["status"].cpu().tolist() == [0, 0, 0, 0, 1, 1]
    for n in range(N):
        want = crop_ref.crop_to_tensor(frames[idx[n]], boxes[n], 1.2) if 0 <= idx[n] < F else np.zeros((3, 224, 224), np.float32)
        np.testing.assert_array_equal(crops[n], want, err_msg=f"crop {n}")
    assert crops[0].max() > 0 and crops[1].max() > 0 and crops[2].min() > 0 and crops[3].max() == 0
    # the 1:1 box really reaches the last frame's last pixel: its value is in the crop
    assert np.float32(frames[1, H - 1, W - 1, 0]) / np.float32(255.0) in crops[1][0]


# ------------------------------------------------------------------------------------------------
# the handles: pr_hmr_forward, pr_hmr_encode_until, pr_frames_forward
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def handles(gpu_device, smpl97):
    sd = synth.hmr_state_dict(seed=1)
    h = {"sd": sd, "oracle": hmr_ref.build(sd), "x": synth.crops(3, seed=4)}
    for precision in ("fp32", "bf16"):
        m = HMR(max_batch=4, precision=precision).to(gpu_device)
        m.load_state_dict(sd)
        h[precision] = m
        h["ref_" + precision] = er.Reference(sd, precision, gpu_device)
    with torch.no_grad():
        p6, b, c = h["oracle"].regress(h["oracle"].features(torch.from_numpy(h["x"])))
        h["want"] = (hmr_ref.rot6d_to_rotmat(p6).view(3, 24, 3, 3).numpy(), b.numpy(), c.numpy())
    h["layer"] = SMPLLayer(smpl97[0], device=gpu_device, max_batch=32)
    return h


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_hmr_forward(gpu_device, handles, precision, B):
    m = handles[precision]

    def call(i, o):
        r, b, c = m(i["x"], out=None if o is None else (o["rotmat"], o["betas"], o["cam"]))
        return {"rotmat": r, "betas": b, "cam": c}

    got = guarded(call, {"x": torch.from_numpy(handles["x"][:B]).to(gpu_device)},
                  {"rotmat": ((B, 24, 3, 3), F32), "betas": ((B, 10), F32), "cam": ((B, 3), F32)})
    r_ref, b_ref, c_ref = (a[:B] for a in handles["want"])
    if precision == "fp32":     # test_hmr_forward_matches_oracle
        np.testing.assert_allclose(got["rotmat"].cpu().numpy(), r_ref, atol=TOL_F32)
        np.testing.assert_allclose(got["betas"].cpu().numpy(), b_ref, atol=TOL_F32)
        np.testing.assert_allclose(got["cam"].cpu().numpy(), c_ref, atol=TOL_F32)
    else:                       # test_hmr_bf16_encoder (the same crops): the stated precision cost of the bf16 encoder
        np.testing.assert_allclose(got["rotmat"].cpu().numpy(), r_ref, atol=5e-2)
        np.testing.assert_allclose(got["betas"].cpu().numpy(), b_ref, atol=5e-2)
        R = got["rotmat"].cpu().numpy().reshape(-1, 3, 3)
        np.testing.assert_allclose(R @ R.transpose(0, 2, 1), np.broadcast_to(np.eye(3), R.shape), atol=1e-5)


# the stem + max-pool; the first and last Bottleneck of layer1 .. layer4 (16, the last, is what the average pool reads)
ENCODER_BLOCKS = [0, 1, 3, 4, 7, 8, 13, 14, 16]


@pytest.mark.parametrize("block", ENCODER_BLOCKS)
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_hmr_encode_until(gpu_device, handles, precision, B, block):
    """The tap's output in a canary arena, the crops in a NaN arena; the value as tests/test_encoder_blocks.py holds it: block
    k against the fp64 reference of block k from the GPU's own tap k - 1, every element within the bound E, no tile's RMS
    of (gpu - ref) / E above RHO times the block's."""
    m, ref = handles[precision], handles["ref_" + precision]
    hw, c = HMR.BLOCK_SHAPES[block]
    x = torch.from_numpy(handles["x"][:B]).to(gpu_device)
    tap = guarded(lambda i, o: {"y": m.encode_until(i["x"], block, out=_o(o, "y"))}, {"x": x},
                  {"y": ((B, hw, hw, c), BF16 if precision == "bf16" else F32)})["y"]
    nchw = lambda t: t.permute(0, 3, 1, 2).double()
    with torch.no_grad():
        if block == 0:
            y, E = ref.block0(x)
        else:
            y, E = ref.block(block, nchw(m.encode_until(x, block - 1)), m.conv_form_resolved() if precision == "fp32" else 0)
    max_r, tile_ratio = er.check_stats(nchw(tap), y, E)
    assert max_r <= 1.0 and tile_ratio <= er.RHO, (max_r, tile_ratio)


def test_frames_forward(gpu_device, handles, smpl97):
    """pr_frames_forward through FramePipeline at B = 3: every output in a canary arena (crop_status is the one buffer of the
    lane the call does not write: a cropping front end points pr_crop_frames' status there), against the oracle pipeline
    as test_pipeline_matches_oracle holds it."""
    B = 3
    info = synth.EXAMPLE_INFO
    pipe = FramePipeline(handles["fp32"], handles["layer"], info, with_verts=True)
    x = torch.from_numpy(handles["x"]).to(gpu_device)
    spec = {k: (tuple(v.shape), v.dtype) for k, v in pipe(x).items()}
    assert set(spec) == {"rotmat", "betas", "cam", "axis_angle", "euler", "joint_cam", "status", "crop_status", "reba", "rula", "verts"}

    def call(i, o):
        return {k: v.clone() for k, v in pipe(i["x"], out=o).items()}

    got = guarded(call, {"x": x}, spec, may_hold_canary=("crop_status",), skip_plain=("crop_status",))
    assert bool((got["crop_status"] == gb.CANARY_I32).all())
    got = {k: v.cpu().numpy() for k, v in got.items()}
    want = pipeline_ref.run(handles["oracle"], smpl97[1], handles["x"], info, batch_size=8)
    for k in ("rotmat", "betas", "cam", "axis_angle"):
        np.testing.assert_allclose(got[k], want[k], atol=TOL_F32)
    d = np.abs(got["euler"] - want["euler"])
    assert np.minimum(d, 360 - d).max() < 2e-2                      # degrees, from 1e-4 rotmat agreement
    np.testing.assert_allclose(got["joint_cam"], want["joint_cam"], atol=TOL_MM)
    assert int(np.abs(got["status"]).sum()) == 0
    np.testing.assert_array_equal(got["reba"], reba_ref.reba_packed(got["euler"], info["REBA"]))
    np.testing.assert_array_equal(got["rula"], rula_ref.rula_packed(got["euler"], info["RULA"]))
    assert np.all(got["axis_angle"][:, 0] == np.array([3.14, 0, 0], np.float32))
    assert np.isfinite(got["verts"]).all() and got["verts"].shape == (B, 97, 3)
