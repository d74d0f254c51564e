"""References and seeded inputs that more than one test module holds the stand-alone kernels against (a helper module, not a
conftest): tests/test_hip_parity.py and tests/test_wino_layer1.py check values with them on plain tensors,
tests/test_guard_band_gpu.py checks the same values with every tensor inside a guard-band arena."""
import numpy as np
import torch
import torch.nn.functional as F

from encoder_ref import _mm
from oracle import coord_ref


def _d(a):
    """numpy array or tensor (any device) -> float64 CPU tensor."""
    return torch.as_tensor(a).cpu().double()


def bf16_round(t):
    return t.to(torch.bfloat16).float()


# ------------------------------------------------------------------------------------------------
# single convolutions
# ------------------------------------------------------------------------------------------------
def conv_ref64(x, w, bias=None, res=None, stride=1, pad=0, relu=False):
    """fp64 conv2d of the NHWC tensor x (its first w.shape[1] channels are real) + bias + residual, ReLU -> NHWC float64."""
    w = _d(w)
    y = F.conv2d(_d(x[..., :w.shape[1]]).permute(0, 3, 1, 2), w, None if bias is None else _d(bias), stride=stride,
                 padding=pad).permute(0, 2, 3, 1)
    if res is not None:
        y = y + _d(res)
    return torch.relu(y) if relu else y


def dual_ref64(t, w1, x, w2, bias, stride2, relu=True):
    """fp64 relu?(t W1^T + x[:, ::s, ::s] W2^T + bias): a first Bottleneck's conv3 with its downsample branch."""
    y = (torch.einsum("bhwc,oc->bhwo", _d(t), _d(w1)) + torch.einsum("bhwc,oc->bhwo", _d(x)[:, ::stride2, ::stride2], _d(w2))
         + _d(bias))
    return torch.relu(y) if relu else y


def assert_close_f32(got, ref, what=""):
    """The fp32 convolutions' criterion: max |got - ref| < 2e-5 max(1, max |ref|)."""
    err = float((_d(got) - ref).abs().max())
    assert err < 2e-5 * max(1.0, float(ref.abs().max())), (what, err)


def assert_close_bf16(got, ref, what=""):
    """A single bf16 convolution's criterion: |got - ref| <= |ref| 2^-8 + 2e-3 elementwise (one bf16 rounding of an fp32 sum)."""
    d = (_d(got.float()) - ref).abs()
    assert bool((d <= ref.abs() * 2.0 ** -8 + 2e-3).all()), (what, float(d.max()))


# ------------------------------------------------------------------------------------------------
# conv2 + conv3 of a layer1 Bottleneck in one kernel
# ------------------------------------------------------------------------------------------------
def fused_ref64(x, w2, b2, w3, b3, res=None, relu=True):
    """fp64 relu?(relu(conv3x3(x, w2) + b2) w3^T + b3 + res) -> NHWC float64."""
    t2 = torch.relu(F.conv2d(_d(x).permute(0, 3, 1, 2), _d(w2), _d(b2), padding=1))
    y = torch.einsum("bchw,oc->bhwo", t2, _d(w3)) + _d(b3)
    if res is not None:
        y = y + _d(res)
    return torch.relu(y) if relu else y


def fused_bf16_emulation(x, w2, b2, w3, b3, res=None):
    """The same in fp32 on bf16-rounded operands (float32 CPU tensors), t2 rounded to bf16 where the kernel stores it."""
    t2 = bf16_round(torch.relu(F.conv2d(x.permute(0, 3, 1, 2), w2, torch.as_tensor(b2), padding=1)))
    y = torch.einsum("bchw,oc->bhwo", t2, w3) + torch.as_tensor(b3)
    if res is not None:
        y = y + res
    return torch.relu(y)


# ------------------------------------------------------------------------------------------------
# layer1's Winograd F(4x4,3x3) kernel (tests/test_wino_layer1.py)
# ------------------------------------------------------------------------------------------------
def wino64_layer(shape, n3=256):
    B, H, W = shape
    rng = np.random.default_rng(1000 * H + W)
    x = rng.standard_normal((B, H, W, 64)).astype(np.float32)
    w2 = (rng.standard_normal((64, 64, 3, 3)) / np.sqrt(64 * 9)).astype(np.float32)
    b2 = rng.standard_normal(64).astype(np.float32)
    w3 = (rng.standard_normal((n3, 64)) / np.sqrt(64)).astype(np.float32)
    b3 = rng.standard_normal(n3).astype(np.float32)
    res = rng.standard_normal((B, H, W, n3)).astype(np.float32)
    return x, w2, b2, w3, b3, res


def wino64_ref64(x, w2, b2, w3=None, b3=None, res=None):
    """fp64: relu(conv3x3(x) + b2) [-> relu(. w3^T + b3 + res)], NHWC numpy."""
    a = torch.from_numpy(x).double().permute(0, 3, 1, 2)
    t2 = torch.relu(_mm(a, torch.from_numpy(w2).double(), 1, 1) + torch.from_numpy(b2).double().view(1, -1, 1, 1))
    if w3 is None:
        return t2.permute(0, 2, 3, 1).numpy()
    y = _mm(t2, torch.from_numpy(w3).double().view(w3.shape[0], 64, 1, 1), 1, 0) + torch.from_numpy(b3).double().view(1, -1, 1, 1)
    return torch.relu(y.permute(0, 2, 3, 1) + torch.from_numpy(res).double()).numpy()


# ------------------------------------------------------------------------------------------------
# whole Bottlenecks in one bf16 kernel
# ------------------------------------------------------------------------------------------------
# input channels, mid channels, and the divisors that keep the three weight matrices' products O(1)
BOTTLENECKS = {64: (256, 64, (16, 24, 8)), 128: (512, 128, (22, 34, 11)), 256: (1024, 256, (32, 48, 16))}


def bottleneck_inputs(mid, case, first=False):
    """Seeded bf16-rounded input and weights (float32 CPU tensors) + fp32 biases of one whole-block case (B, H, W):
    -> x, w1, w2, w3, wd (None unless `first`: the stage's first block, 64-channel input + downsample), biases."""
    B, H, W = case
    cin, _, (s1, s2, s3) = BOTTLENECKS[mid]
    cout = cin
    rng = np.random.default_rng(B * (999 if first else 1000) + H * 10 + W)
    if first:
        cin, s1 = 64, 8
    x = bf16_round(torch.from_numpy(rng.standard_normal((B, H, W, cin)).astype(np.float32)))
    w1 = bf16_round(torch.from_numpy((rng.standard_normal((mid, cin)) / s1).astype(np.float32)))
    w2 = bf16_round(torch.from_numpy((rng.standard_normal((mid, mid, 3, 3)) / s2).astype(np.float32)))
    w3 = bf16_round(torch.from_numpy((rng.standard_normal((cout, mid)) / s3).astype(np.float32)))
    wd = bf16_round(torch.from_numpy((rng.standard_normal((cout, cin)) / 8).astype(np.float32))) if first else None
    biases = tuple(rng.standard_normal(n).astype(np.float32) * 0.5 for n in ((mid, mid, cout, cout) if first else (mid, mid, cout)))
    return x, w1, w2, w3, wd, biases


def bottleneck_emulation(x, w1, b1, w2, b2, w3, b3, wd=None, bd=None):
    """fp32 emulation of the block with t1 and t2 rounded to bf16: relu(conv3(t2) + b3 + x), or for a first block
    relu(conv3(t2) + downsample(x) + (b3 + bd))."""
    e1 = bf16_round(torch.relu(torch.einsum("bhwc,oc->bhwo", x, w1) + torch.from_numpy(b1)))
    e2 = bf16_round(torch.relu(F.conv2d(e1.permute(0, 3, 1, 2), w2, torch.from_numpy(b2), padding=1)))
    if wd is None:
        return torch.relu(torch.einsum("bchw,oc->bhwo", e2, w3) + torch.from_numpy(b3) + x)
    b3d = (b3.astype(np.float64) + bd.astype(np.float64)).astype(np.float32)
    return torch.relu(torch.einsum("bchw,oc->bhwo", e2, w3) + torch.einsum("bhwc,oc->bhwo", x, wd) + torch.from_numpy(b3d))


# ------------------------------------------------------------------------------------------------
# stems
# ------------------------------------------------------------------------------------------------
def stem_pool_bf16_case(case):
    """Seeded input of the bf16 stem kernel and its torch reference: conv in fp32 on the bf16-rounded operands, the map
    rounded to bf16 before the pool -> x, w (float32 CPU tensors), bias, ref NHWC float32."""
    B, H = case
    rng = np.random.default_rng(B * 100 + H)
    x = bf16_round(torch.from_numpy(rng.random((B, H, H, 16)).astype(np.float32)))
    x[..., 12:] = 0                                  # the space-to-depth image has 12 real channels
    w = bf16_round(torch.from_numpy((rng.standard_normal((64, 16, 4, 4)) / 12).astype(np.float32)))
    bias = rng.standard_normal(64).astype(np.float32) * 0.3
    conv = F.conv2d(x.permute(0, 3, 1, 2), w, torch.from_numpy(bias), padding=2)[:, :, :H, :H]
    ref = F.max_pool2d(bf16_round(torch.relu(conv)), 3, stride=2, padding=1).permute(0, 2, 3, 1)
    return x, w, bias, ref


def stem_pool_f32_case(B):
    """Seeded input of the fp32 stem kernel (the 7x7 kernel laid out in the 4x4 taps' 8x8 window, as pr_hmr_create does)
    and its fp64 reference -> x, w, bias (numpy), ref NHWC numpy float64."""
    rng = np.random.default_rng(33)
    x = rng.standard_normal((B, 112, 112, 12)).astype(np.float32)
    # the 7x7 kernel in the 4x4 taps' 8x8 window (a zero row and a zero column in front), as pr_hmr_create lays it out
    w7 = (rng.standard_normal((64, 3, 7, 7)) / np.sqrt(147)).astype(np.float32)
    w = np.zeros((64, 12, 4, 4), np.float32)
    for kh in range(7):
        for kw in range(7):
            th, di, tw, dj = (kh + 1) >> 1, (kh + 1) & 1, (kw + 1) >> 1, (kw + 1) & 1
            w[:, (2 * di + dj) * 3:(2 * di + dj) * 3 + 3, th, tw] = w7[:, :, kh, kw]
    bias = rng.standard_normal(64).astype(np.float32)
    xt = torch.from_numpy(x).permute(0, 3, 1, 2)
    # window rows y-2 .. y+1: pad 2 up/left, 1 down/right
    conv = F.conv2d(F.pad(xt.double(), (2, 1, 2, 1)), torch.from_numpy(w).double(), torch.from_numpy(bias).double())
    ref = F.max_pool2d(torch.relu(conv), 3, 2, 1).permute(0, 2, 3, 1).numpy()
    return x, w, bias, ref, rng


# ------------------------------------------------------------------------------------------------
# rotmat -> axis-angle -> Euler degrees against tests/golden/euler.npz
# ------------------------------------------------------------------------------------------------
def pose_to_euler_errors(ours_aa, ours_eul, gold_aa, gold_eul):
    """-> (d, off, ulp, dg) for the frames given (numpy; golden arrays sliced to the same frames):
    d    Euler degrees against the oracle's Euler stage run on OUR float32 axis-angle (mod 360): the angles are taken from the
         float32 axis-angle, and where ours differs from the reference's by one float32 ulp the angle moves by ~1e-5 deg;
    off  |our axis-angle - the reference's| and ulp, the float32 spacing at the vector's largest component (a component near
         zero carries the absolute error of the others): ours is the reference's or its float32 neighbour (device libm vs
         glibc in the last double ulp of acos / sqrt), i.e. off <= ulp;
    dg   Euler degrees against the reference's own (mod 360), which then move by at most that much."""
    ref = np.stack([coord_ref.axis_angle_to_euler_angle(f) for f in ours_aa])
    d = np.abs(ours_eul - ref)
    d = np.minimum(d, 360 - d)
    big = np.abs(gold_aa).max(axis=2, keepdims=True).astype(np.float32)
    ulp = np.broadcast_to(np.spacing(np.maximum(big, np.float32(1e-30))).astype(np.float64), gold_aa.shape)
    off = np.abs(ours_aa.astype(np.float64) - gold_aa.astype(np.float64))
    dg = np.abs(ours_eul - gold_eul)
    dg = np.minimum(dg, 360 - dg)
    return d, off, ulp, dg
