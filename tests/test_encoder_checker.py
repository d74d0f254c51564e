"""CPU: the per-block checker of tests/test_encoder_blocks.py (tests/encoder_ref.py) accepts a correct route computed in a
different order and rejects the defects a kernel of the bf16 / fp32 encoder could plausibly have."""
import pytest
import torch
import torch.nn.functional as F

import encoder_ref as er
from oracle import hmr_ref


def _block(inplanes, planes, stride, seed):
    """A Bottleneck with BatchNorm statistics that give every channel a bias of its own."""
    torch.manual_seed(seed)
    down = None
    if stride != 1 or inplanes != planes * 4:
        down = torch.nn.Sequential(torch.nn.Conv2d(inplanes, planes * 4, 1, stride=stride, bias=False),
                                   torch.nn.BatchNorm2d(planes * 4))
    blk = hmr_ref.Bottleneck(inplanes, planes, stride, down)
    for m in blk.modules():
        if isinstance(m, torch.nn.Conv2d):
            torch.nn.init.kaiming_normal_(m.weight, mode="fan_out")
        if isinstance(m, torch.nn.BatchNorm2d):
            m.weight.data.uniform_(0.5, 1.5)
            m.bias.data.normal_(0.0, 0.5)
            m.running_mean.data.normal_(0.0, 0.1)
            m.running_var.data.uniform_(0.5, 1.5)
    return blk.eval()


def _conv_f32(c, a, bf16, drop=None):
    """A route's convolution: fp32 products and sums over the K loop in 64-wide steps taken LAST step first, in the packed
    tap-major order k = tap * Cin + ci (conv_k_index_bf16 for one 64-channel slice).  drop = (frame, pixels, channels):
    that output tile misses the last K step."""
    w = c.w.float()
    N, Cin, H, W = a.shape
    k = c.k
    Ho, Wo = (H + 2 * c.pad - k) // c.stride + 1, (W + 2 * c.pad - k) // c.stride + 1
    cols = F.unfold(a.float(), k, padding=c.pad, stride=c.stride)                     # [N, Cin * taps, L] (ci-major)
    cols = cols.view(N, Cin, k * k, -1).transpose(1, 2).reshape(N, k * k * Cin, -1)   # tap-major
    wk = w.permute(0, 2, 3, 1).reshape(w.shape[0], -1)
    acc = torch.zeros(N, w.shape[0], cols.shape[-1])
    steps = list(range(0, wk.shape[1], 64))[::-1]
    for i, k0 in enumerate(steps):
        part = wk[:, k0:k0 + 64] @ cols[:, k0:k0 + 64]
        if drop is not None and i == 0:
            n, px, ch = drop
            part[n, ch, px] = 0
        acc = acc + part
    return (acc + c.b.float().view(1, -1, 1)).view(N, -1, Ho, Wo)


def _route(p, a, bf16, defect=None):
    """The block as a fused route computes it: fp32 accumulation (another order than the reference's), t1 / t2 and the
    output rounded as the plan stores them (bf16 or fp32), the downsample branch in conv3's K loop.  `defect` injects one
    fault."""
    rnd = hmr_ref._bf16 if bf16 else (lambda t: t)
    a = a.float()
    t1 = rnd(_conv_f32(p.c1, a, bf16).clamp_min(0))
    if defect == "halo":   # conv2 reads its input row 3 of frame 0 as zero for output row 4 (a chunk's halo row)
        t1z = t1.clone()
        t1z[0, :, 3] = 0
        z2 = _conv_f32(p.c2, t1, bf16)
        z2[0, :, 4] = _conv_f32(p.c2, t1z, bf16)[0, :, 4]
    else:
        drop = (0, slice(0, 32), slice(0, 32)) if defect == "kstep" else None
        z2 = _conv_f32(p.c2, t1, bf16, drop)
    t2 = rnd(z2.clamp_min(0))
    z3 = _conv_f32(p.c3, t2, bf16)
    if p.cd is not None:
        z3 = z3 + _conv_f32(p.cd, a, bf16)
    else:
        idt = a
        if defect == "residual":   # the ragged last 32-row tile of the GEMM (rows = frames x pixels) misses its residual
            N, C, H, W = a.shape
            rows = idt.permute(0, 2, 3, 1).reshape(N * H * W, C).clone()
            rows[(N * H * W) // 32 * 32:] = 0
            idt = rows.view(N, H, W, C).permute(0, 3, 1, 2)
        z3 = z3 + idt
    if defect == "bias":   # one channel's bias off by BIAS_SHIFT of its magnitude
        c = int(p.c3.b.abs().argmax())
        z3[:, c] += BIAS_SHIFT[bf16] * float(p.c3.b[c].abs())
    return rnd(z3.clamp_min(0)).double()


# 1 % in fp32.  In bf16 a 1 % shift is one to two ulps of the output -- the size of the route's own rounding, caught by
# neither criterion (max |r| 0.09, tile ratio 1.6 against 1.3 for the correct route) -- so bf16 takes 8 %, still inside
# the per-element bound (max |r| 0.64).
BIAS_SHIFT = {False: 0.01, True: 0.08}
CASES = {"plain": (256, 64, 1), "first_s2": (128, 64, 2)}


def _setup(case, bf16):
    inplanes, planes, stride = CASES[case]
    p = er.Block(_block(inplanes, planes, stride, seed=stride), bf16)
    g = torch.Generator().manual_seed(11)
    a = torch.randn(2, inplanes, 9, 9, generator=g).clamp_min(0)
    if bf16:
        a = hmr_ref._bf16(a)
    a = a.double()
    y, E = er.block_ref(p, a, er.U_BF16 if bf16 else er.U_F32)
    return p, a, y, E


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
@pytest.mark.parametrize("case", sorted(CASES))
def test_checker_accepts_a_correct_route(case, precision):
    bf16 = precision == "bf16"
    p, a, y, E = _setup(case, bf16)
    got = _route(p, a, bf16)
    assert not torch.equal(got, y)          # the route really differs from the reference ...
    mx, rms = er.check_stats(got, y, E)
    assert mx <= 1 and rms <= er.RHO, (mx, rms)   # ... and stays inside the bound
    assert mx > (0.01 if bf16 else 1e-6)          # the bound is not loose by orders of magnitude
    if case == "first_s2":
        assert y.shape == (2, 256, 5, 5)


# which criterion each defect trips: "element" = max |r| > 1, "tile" = a tile's RMS of r > RHO x the block's (and
# max |r| <= 1)
DEFECTS = {"kstep": "element", "halo": "element", "residual": "element", "bias": "tile"}


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
@pytest.mark.parametrize("defect", sorted(DEFECTS))
def test_checker_rejects_injected_defects(defect, precision):
    bf16 = precision == "bf16"
    p, a, y, E = _setup("plain", bf16)
    got = _route(p, a, bf16, defect)
    mx, rms = er.check_stats(got, y, E)
    if DEFECTS[defect] == "element":
        assert mx > 1, (mx, rms)
    else:
        assert mx <= 1 and rms > er.RHO, (mx, rms)


def test_tile_rms_localises_a_tile():
    """tile_rms: a defect confined to one 32 x 32 tile shows in that tile only; a ragged frame's last tile averages over
    its own pixels."""
    r = torch.zeros(2, 64, 7, 7, dtype=torch.float64)
    r[1, 32:, 4:, :] = 1.0          # pixels 28..48 of frame 1, channels 32..63
    t = er.tile_rms(r)
    assert t.shape == (2, 2, 2)
    assert t[1, 1, 1] == 1.0        # pixels 32..48: all hit
    assert float(t[1, 0, 1]) == pytest.approx((4 / 32) ** 0.5)    # pixels 0..31: 28..31 hit
    assert float(t.sum()) == pytest.approx(1.0 + (4 / 32) ** 0.5)
